"""The classic front end on the GPU.

python tools/classic_bench.py [frames] [--detector ORB|ShiTomasi|FAST|BRISK|AKAZE] [--descriptor ORB|BRISK|AKAZE|SIFT] [--resident] [--brisk-resident] [--akaze-resident] [--sift-resident] [--orb-octaves] [--octave-pairs-resident] [--sift-octave-pairs-resident] [--orb-brisk] [--orb-pairs-resident] [--sift-brisk] [--sift-brisk-resident]
    ClassicFeatureFrontEnd(detector, descriptor, BF, KNN) over the synthetic stream: frames/s of the synchronous stereoCallback
    (--descriptor BRISK: with --detector ShiTomasi, FAST, BRISK or AKAZE; --detector BRISK: with --descriptor BRISK only; --detector AKAZE:
    with --descriptor BRISK or AKAZE -- the latter sets ClassicFeatureFrontEnd::setAkazeDescriptor for the run: 61-byte MLDB rows);
    --descriptor SIFT: with any of the five detectors (spvo_sift_describe; the per-image path, but see --sift-resident);
    --resident: with ClassicFeatureFrontEnd::setDeviceResident (one spvo_classic_detect per pair, matching on the binary slots);
    --brisk-resident: with setBriskPairResident as well (BRISK + BRISK through one spvo_brisk_detect_pair per pair; needs --resident).
    --akaze-resident: with setAkazePairResident as well (AKAZE + AKAZE through one spvo_akaze_detect_pair per pair; needs --resident).
    --sift-resident: with setSiftDescribeResident as well (ShiTomasi / FAST + SIFT through one spvo_classic_sift_pair per pair; needs --resident;
    also taken by --ab for its resident runs).
    --sift-octave-pairs-resident: with setSiftOctavePairsResident as well (BRISK / AKAZE + SIFT through one spvo_brisk_sift_pair /
    spvo_akaze_sift_pair per pair; needs --resident; also taken by --ab for its resident runs).
    --orb-brisk: with setOrbBriskExtractor (ORB + BRISK runs at all); --orb-pairs-resident: with setOrbPairsResident as well (ORB + BRISK /
    ORB + SIFT through one spvo_orb_brisk_pair / spvo_orb_sift_pair per pair; needs --resident; also taken by --ab for its resident runs).
    --sift-brisk: with setSiftBriskExtractor (--detector SIFT --descriptor BRISK runs at all); --sift-brisk-resident: with setSiftBriskResident
    as well (SIFT + BRISK through one spvo_sift_brisk_pair per pair; needs --resident; also taken by --ab for its resident runs).
python tools/classic_bench.py [frames] --detector ShiTomasi|FAST|ORB|BRISK|AKAZE|SIFT --descriptor ORB|BRISK|SIFT --ab ROUNDS [--sift-resident] [--sift-octave-pairs-resident] [--orb-brisk] [--orb-pairs-resident] [--sift-brisk] [--sift-brisk-resident] [--waves N]
    the same stream with setDeviceResident off and on, alternating, ROUNDS times each in one process: ms per pair of every run, the median
    and the min .. max spread of each setting, and how many pairs of a resident run stayed resident.  --waves N: tuning
    "sift_pair_waves_per_cu" = N for the SIFT pair calls of the resident runs.
python tools/classic_bench.py --detectors [--calls 200] [--warmup 20]
    per image at 1241 x 376: spvo_orb_detect (the yardstick, same run) beside spvo_gftt_detect + spvo_orb_describe and
    spvo_fast_detect + spvo_orb_describe -- median, 10th / 90th percentile of the synchronous calls, keypoints, and how the
    minimum-distance iteration went (undecided candidates after each round launch, rounds of the finish kernel).
python tools/classic_bench.py --leg gftt|fast|orb|sift [--calls 50]
    one leg alone, for rocprofv3 --kernel-trace --stats -- python tools/classic_bench.py --leg gftt
    (sift: spvo_sift_detect per image at 1241 x 376; the per-kernel split -- sift_blur_kernel / sift_extrema_kernel / sift_refine_kernel /
    sift_describe_kernel -- is the kernel trace's)
python tools/classic_bench.py --leg brisk|orb_describe [--calls 50]
    spvo_brisk_describe / spvo_orb_describe alone on the FAST keypoints of the 1241 x 376 sample (image passed with every call), for
    rocprofv3 --kernel-trace --stats as above: brisk_integral_rows_kernel + brisk_integral_cols_kernel / brisk_compact_kernel /
    brisk_describe_kernel is the split.  --leg brisk also prints the one-off cost: the table build and the first call's upload.
python tools/classic_bench.py --leg orb_octaves [--calls 100]
    spvo_orb_describe_octaves alone on the BRISK detector's keypoints (octaves 0..5) of the 1241 x 376 sample, image passed with every
    call and on the resident image (img = NULL), for rocprofv3 --kernel-trace --stats as above (orb_resize_kernel x top octave /
    orb_blur_h_kernel / orb_blur_v_kernel / orb_describe_given_kernel is the split), and in the same run its yardstick:
    spvo_orb_describe on the FAST keypoints of the same image.  The whole pair through the host class: --detector BRISK|AKAZE
    --descriptor ORB --orb-octaves (ClassicFeatureFrontEnd::setOrbExtractorOctaves for the run).
python tools/classic_bench.py --leg brisk_detect [--calls 50]
    spvo_brisk_detect (threshold 30) alone per image at 1241 x 376, for rocprofv3 --kernel-trace --stats as above: brisk_area_kernel /
    brisk_half_kernel / brisk_score916_kernel / brisk_score58_kernel / brisk_collect_kernel / cls_rank_kernel / brisk_refine_kernel /
    brisk_det_compact_kernel is the split.
python tools/classic_bench.py --leg akaze_detect [--calls 50] [--yardstick]
    spvo_akaze_detect (threshold 0.001) alone per image at 1241 x 376, for rocprofv3 --kernel-trace --stats as above: akaze_blur_kernel /
    akaze_half_kernel or akaze_area_kernel / akaze_gradmax_kernel / akaze_hist_kernel / akaze_contrast_finish_kernel / akaze_flow_kernel /
    akaze_fed_kernel / akaze_deriv_kernel / akaze_det_kernel / akaze_extrema_kernel / cls_rank_kernel / akaze_refine_kernel is the split.
    Prints the launches of one call (from spvo_akaze_tables); --yardstick: spvo_sift_detect afterwards in the same run.
python tools/classic_bench.py --leg akaze_describe [--calls 100]
    spvo_akaze_describe alone on the detector's keypoints of the 1241 x 376 sample, for rocprofv3 --kernel-trace --stats as above
    (akaze_describe_kernel: one launch), and in the same run its yardsticks: spvo_brisk_describe(img = NULL) on the same keypoints,
    spvo_akaze_describe with the image passed (the scale space rebuilt: the detector's chain without its extrema), spvo_akaze_detect.
python tools/classic_bench.py --leg brisk_pair [--calls 50]
    spvo_brisk_detect_pair (threshold 30) alone on the 1241 x 376 sample pair, rotating through the slot ring, for rocprofv3 --kernel-trace
    --stats as above: the detector's kernels up to brisk_refine_kernel, then brisk_integral_*_kernel / brisk_pair_compact_kernel /
    brisk_describe_kernel / brisk_pair_finish_kernel, twice per call.
python tools/classic_bench.py --leg akaze_pair [--calls 100]
    spvo_akaze_detect_pair (threshold 0.001) alone on the 1241 x 376 sample pair -- BOTH images per call -- rotating through the slot ring,
    for rocprofv3 --kernel-trace --stats as above: the detector's kernels up to akaze_refine_kernel, then akaze_suppress_first_kernel /
    akaze_suppress_second_kernel / akaze_suppress_compact_kernel / akaze_describe_kernel / akaze_pair_finish_kernel, twice per call.
    Its yardsticks are --leg akaze_detect and --leg akaze_describe: two per-image detects plus two describes.
python tools/classic_bench.py --leg brisk_orb_pair|akaze_orb_pair|akaze_brisk_pair [--calls 100]
    spvo_brisk_orb_pair / spvo_akaze_orb_pair / spvo_akaze_brisk_pair on the 1241 x 376 sample pair -- BOTH images per call -- rotating
    through the slot ring, and ALTERNATING with it call by call in the same run its yardstick, the per-image sequence of both images:
    spvo_brisk_detect / spvo_akaze_detect, then spvo_orb_describe_octaves(img = NULL) / spvo_brisk_describe(img = NULL) on its keypoints.
    For rocprofv3 --kernel-trace --stats as above (--no-yardstick: the pair call alone): behind the detector's kernels
    orb_link_group_kernel / orb_resize_kernel x max octave / orb_blur_h_kernel / orb_blur_v_kernel / orb_link_describe_kernel /
    orb_link_finish_kernel, or akaze_present_brisk_kernel / brisk_integral_*_kernel / brisk_pair_compact_kernel / brisk_describe_kernel /
    brisk_pair_finish_kernel / akaze_brisk_finish_kernel, twice per call.  The whole pair through the host class: --detector BRISK|AKAZE
    --descriptor ORB|BRISK [--orb-octaves] --resident --octave-pairs-resident (ClassicFeatureFrontEnd::setOctavePairsResident for the run).
python tools/classic_bench.py --leg orb_brisk_pair|orb_sift_pair [--calls 100]
    spvo_orb_brisk_pair / spvo_orb_sift_pair on the 1241 x 376 sample pair -- BOTH images per call -- rotating through the slot ring, and
    ALTERNATING with it call by call in the same run its yardstick, the per-image route of both images: spvo_orb_detect, the records
    converted on the host, then spvo_brisk_describe / spvo_sift_describe with the image passed again (spvo_orb_detect leaves none
    resident).  For rocprofv3 --kernel-trace --stats as above (--no-yardstick: the pair call alone): behind spvo_orb_detect's kernels
    orb_records_kernel, then brisk_integral_*_kernel / brisk_pair_compact_kernel / brisk_describe_kernel / brisk_pair_finish_kernel, or
    sift_blur_kernel x the reduced pyramid / sift_describe_given_kernel, twice per call.  The whole pair through the host class:
    --detector ORB --descriptor BRISK|SIFT [--orb-brisk] --resident --orb-pairs-resident, or --ab.
python tools/classic_bench.py --leg sift_brisk_pair [--calls 100]
    spvo_sift_brisk_pair on the 1241 x 376 sample pair -- BOTH images per call -- rotating through the slot ring, and ALTERNATING with it
    call by call in the same run its yardstick, the per-image route of both images: spvo_sift_detect (with its 128-float rows), then
    spvo_brisk_describe at the records' x, y, size with the image passed again (spvo_sift_detect leaves none resident).  For rocprofv3
    --kernel-trace --stats as above (--no-yardstick: the pair call alone): sift_blur_kernel x the pyramid / sift_extrema_kernel /
    sift_refine_kernel / sift_describe_kernel<false> / sift_key_kernel / sift_rank_kernel / sift_unique_kernel / sift_records_kernel, then
    brisk_integral_*_kernel / brisk_pair_compact_kernel / brisk_describe_kernel / brisk_pair_finish_kernel, twice per call.  The whole
    pair through the host class: --detector SIFT --descriptor BRISK --sift-brisk --resident --sift-brisk-resident, or --ab.
python tools/classic_bench.py --leg fast_sift|gftt_sift|sift_describe [--calls 50] [--form 0|1] [--yardstick] [--sift-resident]
    FAST + SIFT per image at 1241 x 376, for rocprofv3 --kernel-trace --stats as above.  sift_describe: spvo_sift_describe alone on the FAST
    keypoints of the sample (size 7, angle -1, octave 0; image passed with every call): sift_blur_kernel x 6 / sift_describe_given_kernel is
    the split.  fast_sift: spvo_fast_detect + spvo_sift_describe(img = NULL), what ClassicFeatureFrontEnd(FAST, SIFT) runs per image.
    --form 1: tuning "sift_describe_form" = 1, the staged form of the sums instead of the columns.  --yardstick (fast_sift): afterwards, in the
    same run, ms per pair through the host class for FAST + SIFT, SIFT + SIFT and FAST + BRISK over the synthetic stream.
    gftt_sift: the same with spvo_gftt_detect and size 5.  --sift-resident (fast_sift, gftt_sift): the leg is ONE spvo_classic_sift_pair on the
    sample pair -- BOTH images per call, rotating through the slot ring -- instead of the two per-image calls: the detector's kernels, one
    sift_blur_kernel and sift_describe_given_kernel, twice per call; with --yardstick the host class runs that detector + SIFT with
    setDeviceResident and setSiftDescribeResident and says how many pairs stayed resident.  --waves N: tuning "sift_pair_waves_per_cu" = N,
    the descriptor kernel's fixed grid of N waves per CU instead of the default.
python tools/classic_bench.py --leg match|match_slots [--selector NN|KNN] [--cross] [--calls 50]
    one matcher alone on the two resident ORB sets of the 1241 x 376 sample pair: spvo_match_hamming on the host copies (match_hamming_kernel<8>)
    or spvo_match_hamming_slots on the binary slots (match_hamming_tiled_kernel), for rocprofv3 --kernel-trace --stats as above.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "superpoint-stereo-visual-odometry_amd"))
import numpy as np
from spvo import capi, host, synth

ap = argparse.ArgumentParser()
ap.add_argument("frames", nargs="?", type=int, default=60)
ap.add_argument("--detector", default="ORB")
ap.add_argument("--descriptor", default="ORB")
ap.add_argument("--detectors", action="store_true")
ap.add_argument("--resident", action="store_true")
ap.add_argument("--brisk-resident", action="store_true")
ap.add_argument("--akaze-resident", action="store_true")
ap.add_argument("--sift-resident", action="store_true")
ap.add_argument("--orb-octaves", action="store_true")
ap.add_argument("--octave-pairs-resident", action="store_true")
ap.add_argument("--sift-octave-pairs-resident", action="store_true")
ap.add_argument("--orb-brisk", action="store_true")
ap.add_argument("--orb-pairs-resident", action="store_true")
ap.add_argument("--sift-brisk", action="store_true")
ap.add_argument("--sift-brisk-resident", action="store_true")
ap.add_argument("--no-yardstick", action="store_true")
ap.add_argument("--ab", type=int, default=0)
ap.add_argument("--leg", choices=["gftt", "fast", "orb", "sift", "brisk", "brisk_detect", "akaze_detect", "akaze_describe", "akaze_pair", "brisk_pair", "brisk_orb_pair", "akaze_orb_pair", "akaze_brisk_pair", "orb_brisk_pair", "orb_sift_pair", "sift_brisk_pair", "orb_describe", "orb_octaves", "fast_sift", "gftt_sift", "sift_describe", "match", "match_slots"])
ap.add_argument("--form", type=int, default=0, choices=[0, 1])
ap.add_argument("--waves", type=int, default=0)
ap.add_argument("--selector", default="KNN", choices=["NN", "KNN"])
ap.add_argument("--cross", action="store_true")
ap.add_argument("--yardstick", action="store_true")
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
args = ap.parse_args()
frames, poses, P_l, P_r = synth.stereo_sequence(8, os.path.join(ROOT, "tests", "golden", "images", "0000000000.png"), seed=0)

if args.detectors or args.leg:
    img = np.ascontiguousarray(frames[0][0][:376, :1241])
    ctx = capi.Context(net_height=64, net_width=96)

    def leg_orb():
        return len(ctx.orb(img)["xy"])

    def leg_gftt():
        g = ctx.gftt(img)
        return len(ctx.orb_describe(None, g["xy"])["kept"])

    def leg_fast():
        g = ctx.fast(img)
        return len(ctx.orb_describe(None, g["xy"])["kept"])

    def leg_sift():
        return ctx.sift_detect(img)["n"]

    if args.leg in ("fast_sift", "gftt_sift", "sift_describe"):
        capi.set_tuning("sift_describe_form", args.form)
        if args.waves > 0:
            capi.set_tuning("sift_pair_waves_per_cu", args.waves)

    def fast_records(f, size=7.0):                     # KeyPoint(x, y, 7.f, -1, score), octave 0 (Shi-Tomasi: size 5)
        rec = np.zeros(len(f["xy"]), capi.SIFT_KP_DTYPE)
        rec["x"], rec["y"], rec["size"], rec["angle"], rec["response"] = f["xy"][:, 0], f["xy"][:, 1], size, -1.0, f["response"]
        return rec

    if args.leg == "sift_describe":
        srec = fast_records(ctx.fast(img))

    def leg_sift_describe():
        return len(ctx.sift_describe(img, srec))

    def leg_fast_sift():
        return len(ctx.sift_describe(None, fast_records(ctx.fast(img)), shape=img.shape))

    def leg_gftt_sift():
        return len(ctx.sift_describe(None, fast_records(ctx.gftt(img), 5.0), shape=img.shape))

    def leg_sift_pair():                               # --sift-resident: both images in one call
        k = pair_calls[0] % 4
        pair_calls[0] += 1
        fl, fr = ctx.classic_sift_pair(img, pair_r, 2 * k, 2 * k + 1, kind="FAST" if args.leg == "fast_sift" else "ShiTomasi")
        return fl["n"] + fr["n"]

    if args.leg in ("brisk", "orb_describe", "orb_octaves"):
        kp = ctx.fast(img)["xy"]
        if args.leg == "brisk":
            t0 = time.perf_counter()
            capi.brisk_tables(scales=())
            t1 = time.perf_counter()
            ctx.brisk_describe(img, kp, 7.0)
            t2 = time.perf_counter()
            print("BRISK one-off: table build %.1f ms; first spvo_brisk_describe of the context (47 MB table upload, buffers) %.1f ms" % (1e3 * (t1 - t0), 1e3 * (t2 - t1)))

    def leg_brisk():
        return len(ctx.brisk_describe(img, kp, 7.0)["kept"])

    def leg_brisk_detect():
        return ctx.brisk_detect(img, 30)["n"]

    def leg_akaze_detect():
        return ctx.akaze_detect(img)["n"]

    if args.leg == "akaze_describe":
        akp = ctx.akaze_detect(img)["kp"]
        axy = np.ascontiguousarray(np.stack([akp["x"], akp["y"]], 1))

    def leg_akaze_describe():                          # on the scale space the last detect / describe(img) left
        return len(ctx.akaze_describe(None, akp)["desc"])

    def leg_akaze_brisk_null():                        # the yardstick: the BRISK extractor on the same keypoints, image resident
        return len(ctx.brisk_describe(None, axy, akp["size"], shape=img.shape)["kept"])

    def leg_akaze_describe_img():                      # the scale space rebuilt first
        return len(ctx.akaze_describe(img, akp)["desc"])

    if args.leg == "akaze_detect":
        T = capi.akaze_tables(*img.shape)
        new_octaves = int((np.diff(T["octave"]) > 0).sum())
        # level 0 and the contrast factor: memset + 5; per transition blur + flow + its steps (+ the half-sampling); per level 2; extrema per
        # octave with room inside the 29-pixel border, rank, refine
        roomy = sum(1 for o in range(int(T["octave"].max()) + 1) if int(img.shape[0] / 2 ** o) > 58 and int(img.shape[1] / 2 ** o) > 58)
        print("spvo_akaze_detect %d x %d: %d levels, %d diffusion steps, %d kernel launches and 1 memset per call" % (
            img.shape[1], img.shape[0], len(T["octave"]), len(T["tau"]), 5 + 2 * (len(T["octave"]) - 1) + len(T["tau"]) + new_octaves + 2 * len(T["octave"]) + roomy + 2))

    pair_calls = [0]

    def leg_brisk_pair():
        k = pair_calls[0] % 4
        pair_calls[0] += 1
        fl, fr = ctx.brisk_detect_pair(img, pair_r, 2 * k, 2 * k + 1, 30)
        return fl["n"] + fr["n"]

    def leg_akaze_pair():
        k = pair_calls[0] % 4
        pair_calls[0] += 1
        fl, fr = ctx.akaze_detect_pair(img, pair_r, 2 * k, 2 * k + 1)
        return fl["n"] + fr["n"]

    ORB_PAIRS = ("orb_brisk_pair", "orb_sift_pair")
    OCTAVE_PAIRS = ("brisk_orb_pair", "akaze_orb_pair", "akaze_brisk_pair", "sift_brisk_pair") + ORB_PAIRS
    if args.leg in ("brisk_pair", "akaze_pair", "fast_sift", "gftt_sift") + OCTAVE_PAIRS:
        pair_r = np.ascontiguousarray(frames[0][1][:376, :1241])

    def leg_octave_pair():                             # both images in one call
        k = pair_calls[0] % 4
        pair_calls[0] += 1
        fl, fr = getattr(ctx, args.leg)(img, pair_r, 2 * k, 2 * k + 1)
        return fl["n"] + fr["n"]

    def orb_records(o):                                # the host's to_keypoint: size 31 x 1.2^octave (repeated float product), degrees 0 .. 360
        scale = np.ones(8, np.float32)
        for l in range(1, 8):
            scale[l] = scale[l - 1] * np.float32(1.2)
        rec = np.zeros(len(o["xy"]), capi.SIFT_KP_DTYPE)
        deg = o["angle"] * np.float32(57.29577951308232)
        rec["x"], rec["y"], rec["size"], rec["response"], rec["octave"] = o["xy"][:, 0], o["xy"][:, 1], np.float32(31) * scale[o["octave"] & 7], o["response"], o["octave"]
        rec["angle"] = np.where(deg < 0, deg + np.float32(360), deg)
        return rec

    def leg_octave_pair_per_image():                   # its yardstick: detector, then the extractor on the resident image, per image
        n = 0
        for im in (img, pair_r):
            if args.leg in ORB_PAIRS:                  # (spvo_orb_detect leaves no image resident: the extractor takes it again)
                rec = orb_records(ctx.orb(im))
                n += len(ctx.sift_describe(im, rec)) if args.leg == "orb_sift_pair" else len(ctx.brisk_describe(im, np.stack([rec["x"], rec["y"]], 1), rec["size"])["kept"])
                continue
            if args.leg == "sift_brisk_pair":          # (spvo_sift_detect keeps an image of its own: the extractor takes it again)
                rec = ctx.sift_detect(im)["kp"]
                n += len(ctx.brisk_describe(im, np.stack([rec["x"], rec["y"]], 1), rec["size"])["kept"])
                continue
            kp = (ctx.brisk_detect(im, 30) if args.leg == "brisk_orb_pair" else ctx.akaze_detect(im))["kp"]
            xy = np.stack([kp["x"], kp["y"]], 1)
            d = ctx.brisk_describe(None, xy, kp["size"], shape=im.shape) if args.leg == "akaze_brisk_pair" else ctx.orb_describe_octaves(None, xy, kp["octave"], shape=im.shape)
            n += len(d["kept"])
        return n

    def leg_orb_describe():
        return len(ctx.orb_describe(img, kp)["kept"])

    if args.leg == "orb_octaves":
        bkp = ctx.brisk_detect(img, 30)["kp"]
        bxy = np.ascontiguousarray(np.stack([bkp["x"], bkp["y"]], 1))
        print("BRISK keypoints %d, per octave %s" % (len(bkp), np.bincount(bkp["octave"], minlength=6).tolist()))

    def leg_orb_octaves():
        return len(ctx.orb_describe_octaves(img, bxy, bkp["octave"])["kept"])

    def leg_orb_octaves_null():                        # on the image the call before left resident
        return len(ctx.orb_describe_octaves(None, bxy, bkp["octave"], shape=img.shape)["kept"])

    if args.leg in ("match", "match_slots"):
        img_r = np.ascontiguousarray(frames[0][1][:376, :1241])
        fl, fr = ctx.classic_detect(img, img_r, 0, 1, "ORB")

        def leg_match():
            return int((ctx.match_hamming(fl["desc"], fr["desc"], args.selector, args.cross, 0.8)[0] >= 0).sum())

        def leg_match_slots():
            return int((ctx.match_hamming_slots(0, 1, args.selector, args.cross, 0.8)[0] >= 0).sum())

    else:
        leg_match = leg_match_slots = None

    legs = dict(match=("spvo_match_hamming, %d x %d rows" % (len(fl["xy"]) if leg_match else 0, len(fr["xy"]) if leg_match else 0), leg_match),
                match_slots=("spvo_match_hamming_slots, %d x %d rows" % (len(fl["xy"]) if leg_match else 0, len(fr["xy"]) if leg_match else 0), leg_match_slots),
                brisk=("spvo_brisk_describe, %d FAST keypoints" % (len(kp) if args.leg == "brisk" else 0), leg_brisk),
                orb_describe=("spvo_orb_describe, %d FAST keypoints" % (len(kp) if args.leg in ("orb_describe", "orb_octaves") else 0), leg_orb_describe),
                orb_octaves=("spvo_orb_describe_octaves(img), BRISK keypoints", leg_orb_octaves), orb_octaves_null=("spvo_orb_describe_octaves(NULL), BRISK keypoints", leg_orb_octaves_null),
                akaze_describe=("spvo_akaze_describe(NULL)", leg_akaze_describe), akaze_brisk_null=("spvo_brisk_describe(NULL), same keypoints", leg_akaze_brisk_null),
                akaze_describe_img=("spvo_akaze_describe(img)", leg_akaze_describe_img),
                brisk_detect=("spvo_brisk_detect", leg_brisk_detect), akaze_detect=("spvo_akaze_detect", leg_akaze_detect), brisk_pair=("spvo_brisk_detect_pair (both images)", leg_brisk_pair),
                akaze_pair=("spvo_akaze_detect_pair (both images)", leg_akaze_pair),
                octave_pair=("spvo_%s (both images)" % args.leg, leg_octave_pair), octave_pair_per_image=("its per-image sequence (both images)", leg_octave_pair_per_image),
                sift_describe=("spvo_sift_describe, %d FAST keypoints, form %d" % (len(srec) if args.leg == "sift_describe" else 0, args.form), leg_sift_describe),
                fast_sift=("spvo_fast_detect + spvo_sift_describe(NULL), form %d" % args.form, leg_fast_sift),
                gftt_sift=("spvo_gftt_detect + spvo_sift_describe(NULL), form %d" % args.form, leg_gftt_sift),
                orb=("spvo_orb_detect", leg_orb), sift=("spvo_sift_detect", leg_sift), gftt=("spvo_gftt_detect + spvo_orb_describe", leg_gftt), fast=("spvo_fast_detect + spvo_orb_describe", leg_fast))
    if args.sift_resident and args.leg in ("fast_sift", "gftt_sift"):
        legs[args.leg] = ("spvo_classic_sift_pair (%s, both images)" % ("FAST" if args.leg == "fast_sift" else "ShiTomasi"), leg_sift_pair)
    keys = [args.leg] + (["sift"] if args.yardstick and args.leg not in ("fast_sift", "gftt_sift") else []) if args.leg else ["orb", "gftt", "fast"]
    if args.leg == "akaze_describe":
        keys = ["akaze_describe", "akaze_brisk_null", "akaze_describe_img", "akaze_detect"]
    if args.leg == "orb_octaves":
        keys = ["orb_octaves", "orb_octaves_null", "orb_describe"]
    if args.leg in OCTAVE_PAIRS:                       # the two sides alternate call by call
        keys = ["octave_pair"] + ([] if args.no_yardstick else ["octave_pair_per_image"])
        alt, counts = {k: [] for k in keys}, {}
        for i in range(args.warmup + args.calls):
            for k in keys:
                t0 = time.perf_counter()
                counts[k] = legs[k][1]()
                if i >= args.warmup:
                    alt[k].append(1e3 * (time.perf_counter() - t0))
    for key in keys:
        name, fn = legs[key]
        if args.leg in OCTAVE_PAIRS:
            ts, n = alt[key], counts[key]
        else:
            for _ in range(args.warmup):
                n = fn()
            ts = []
            for _ in range(args.calls):
                t0 = time.perf_counter()
                n = fn()
                ts.append(1e3 * (time.perf_counter() - t0))
        ts = np.array(ts)
        extra = ""
        if key == "gftt":
            rem, fin = ctx.gftt_rounds()
            extra = ", undecided after the round launches %s, finish rounds %d" % (rem.tolist(), fin)
        print("%-40s %d x %d: median %.3f ms (p10 %.3f, p90 %.3f) over %d calls, %d described keypoints / matches%s" % (name, img.shape[1], img.shape[0], np.median(ts), np.percentile(ts, 10),
                                                                                                      np.percentile(ts, 90), args.calls, n, extra))
    ctx.close()
    if args.leg in ("fast_sift", "gftt_sift") and args.yardstick:     # the host class, ms per pair, in the same run
        seq = [frames[i % 8] for i in range(args.frames)]
        own = "FAST" if args.leg == "fast_sift" else "ShiTomasi"
        res = dict(resident=True, sift_describe_resident=True) if args.sift_resident else {}
        for det, des in ((own, "SIFT"),) if args.sift_resident or own != "FAST" else (("FAST", "SIFT"), ("SIFT", "SIFT"), ("FAST", "BRISK")):
            host.classic_sequence(seq[:3], P_l, P_r, "KNN", True, 2.0, 4, detector=det, descriptor=des, **res)      # the one-off costs
            p, s, sec = host.classic_sequence(seq, P_l, P_r, "KNN", True, 2.0, 4, warm=5, detector=det, descriptor=des, **res)
            print("host class %s + %s %dx%d: %.3f ms per pair over %d pairs, keypoints %d, stereo matches %d, inliers %d, %d pairs resident" % (
                det, des, frames[0][0].shape[1], frames[0][0].shape[0], 1e3 * sec / (len(seq) - 5), len(seq) - 5, np.median(s[5:, 0]), np.median(s[5:, 2]), np.median(s[5:, 3]),
                host.classic_resident_pairs()))
    capi.set_tuning("sift_describe_form", 0)
elif args.ab > 0:
    if args.waves > 0:
        capi.set_tuning("sift_pair_waves_per_cu", args.waves)
    n = args.frames
    seq = [frames[i % 8] for i in range(n)]
    name = args.detector + ("" if args.descriptor == "ORB" else " + " + args.descriptor)
    ms = {False: [], True: []}
    host.classic_sequence(seq[:8], P_l, P_r, "KNN", True, 2.0, 4, detector=args.detector, descriptor=args.descriptor, orb_brisk=args.orb_brisk, sift_brisk=args.sift_brisk)      # the process's one-off costs
    for r in range(args.ab):
        for resident in (False, True):
            p, s, sec = host.classic_sequence(seq, P_l, P_r, "KNN", True, 2.0, 4, warm=5, detector=args.detector, resident=resident, descriptor=args.descriptor,
                                                sift_describe_resident=resident and args.sift_resident,
                                                sift_octave_pairs_resident=resident and args.sift_octave_pairs_resident, orb_brisk=args.orb_brisk,
                                                orb_pairs_resident=resident and args.orb_pairs_resident, sift_brisk=args.sift_brisk,
                                                sift_brisk_resident=resident and args.sift_brisk_resident)
            ms[resident].append(1e3 * sec / (n - 5))
            print("%s %dx%d round %d resident=%d: %.3f ms per pair over %d pairs, %d pairs resident, keypoints %d, stereo matches %d, inliers %d" % (
                name, frames[0][0].shape[1], frames[0][0].shape[0], r, resident, ms[resident][-1], n - 5, host.classic_resident_pairs(), np.median(s[5:, 0]), np.median(s[5:, 2]), np.median(s[5:, 3])))
    for resident in (False, True):
        v = np.array(ms[resident])
        print("%s resident=%d: median %.3f ms per pair (min %.3f, max %.3f over %d runs)" % (name, resident, np.median(v), v.min(), v.max(), len(v)))
    print("%s resident / per-image = %.3f" % (name, np.median(ms[True]) / np.median(ms[False])))
else:
    n = args.frames
    seq = [frames[i % 8] for i in range(n)]
    p, s, sec = host.classic_sequence(seq, P_l, P_r, "KNN", True, 2.0, 4, warm=5, detector=args.detector, resident=args.resident, descriptor=args.descriptor,
                                        akaze_descriptor=args.descriptor == "AKAZE", **(dict(brisk_resident=True) if args.brisk_resident else {}), **(dict(akaze_resident=True) if args.akaze_resident else {}),
                                        **(dict(sift_describe_resident=True) if args.sift_resident else {}), **(dict(orb_octaves=True) if args.orb_octaves else {}),
                                        **(dict(octave_pairs_resident=True) if args.octave_pairs_resident else {}),
                                        **(dict(sift_octave_pairs_resident=True) if args.sift_octave_pairs_resident else {}), orb_brisk=args.orb_brisk,
                                        orb_pairs_resident=args.orb_pairs_resident, sift_brisk=args.sift_brisk, sift_brisk_resident=args.sift_brisk_resident)
    print("classic front end (%s%s) on the GPU: %.1f stereo frames/s (%.3f ms per pair), keypoints %d, stereo matches %d, inliers %d, %d pairs resident" % (args.detector + ("" if args.descriptor == "ORB" else " + " + args.descriptor), ", device-resident" if args.resident else "", (n - 5) / sec, 1e3 * sec / (n - 5), np.median(s[5:, 0]), np.median(s[5:, 2]), np.median(s[5:, 3]), host.classic_resident_pairs()))
