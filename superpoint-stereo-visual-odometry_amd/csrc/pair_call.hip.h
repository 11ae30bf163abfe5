// pair_call.hip.h -- the resident stereo-pair protocol, written once: what every entry point that takes a stereo pair, fills two device
// slots and returns after one wait does around its own per-image chains (spvo_classic_detect; spvo_brisk_detect_pair and spvo_akaze_detect_pair
// with their ORB / BRISK extractor variants; spvo_orb_brisk_pair; spvo_sift_detect_pair, spvo_classic_sift_pair and sift_link_pair).  Host code only.
//
// A call is a PairCall<Family> whose methods are the protocol's phases, in this order; the caller's own refusals, allocations and chains
// stand between them as ordinary code:
//   check, check_capacity   bad slots / output buffers, the capacity limit                       } nothing on the device or in the slots is
//   (the caller's refusals of its parameters and of the shape)                                   } touched by a refused call
//   open                    require_idle, hipSetDevice, the outputs' counts zeroed
//   (the caller's `ensure`s: EVERY allocation, the family's slots among them, precedes the first launch)
//   load                    both slots rewritten, the prematch cache invalidated, the temporal partner chosen, the solver's stream
//                           synchronised, both images staged in pinned memory (image(k))
//   (the caller's chains, left image then right image, in stream order)
//   submit                  ev_feat recorded, the two prematches enqueued behind it, the ONE wait of the call
//   count(k)                image k's rows from the pinned mirror into the caller's struct (the caller's detector-overflow rule goes here:
//                           its status code and text are the entry point's own)
//   commit                  the capacity rule, the slots filled, min(n, cap) rows copied out, the prematches recorded, last_slot_l set
//
// What differs between the binary slots (BinPairFamily, below) and the SIFT slots (SiftPairFamily, spvo_sift.hip) is the Family:
//   SLOTS, CAP_MAX          the slot ring's size and the rows a slot may be asked to hold
//   OUT_NEEDS_BUFFERS       whether an output struct with cap > 0 must carry both buffers (SIFT) or may leave kp / desc NULL (binary)
//   pair, h_n, slot         the family's PairStage, its pinned [2][4] count block and its slots in spvo_ctx
//   rewrite, partner_ok     a slot is being rewritten; a previous left slot is an acceptable temporal partner (filled; binary: of this row width)
//   FORGETS_AFTER_WAIT      the point where the temporal partner is forgotten.  Binary: after the wait (a call that failed before it leaves
//                           the partner it found).  SIFT: before staging (a call that fails from then on leaves none).  The two differ only
//                           when a call dies of a device or allocation error mid-way; each family keeps the point it has always had.
//   before_chains           SIFT: the chains wait for ev_match, since a match of an earlier call may still read the slots where the L2 matcher
//                           runs.  Binary: nothing, its matcher runs on the chains' own stream.
//   enqueue_prematch, record_prematch   how spvo_set_prematch's two matches are enqueued behind ev_feat and where their results will be
#pragma once
#include "spvo_internal.hip.h"

#pragma GCC visibility push(hidden)
namespace spvo_int {

// the pinned mirrors of one image that commit copies rows from: records of kp_bytes each (NULL: the caller converts them itself) and rows of row_bytes
struct PairMirror { const void *kp; size_t kp_bytes; const void *desc; size_t row_bytes; };

template <class F>
struct PairCall {
  spvo_ctx *c;
  const char *who;           // the entry point, for the error texts
  F f;
  PairOut out[2];
  int slots[2] = {-1, -1}, partner[2] = {-1, -1};   // partner: [stereo, temporal or -1]
  int cap = 0;               // rows a slot holds for this call's capacity rule (check_capacity: the caller's slot_capacity)
  size_t px = 0;

  PairCall(spvo_ctx *ctx, const char *name, const F &family, const PairOut &out_l, const PairOut &out_r) : c(ctx), who(name), f(family), out{out_l, out_r} {}

  int check(int slot_l, int slot_r) {
    if (slot_l < 0 || slot_l >= F::SLOTS || slot_r < 0 || slot_r >= F::SLOTS || slot_l == slot_r) return fail(c, SPVO_ERR_INVALID, "bad slot");
    for (const PairOut &o : out)
      if (o.cap < 0 || (F::OUT_NEEDS_BUFFERS && o.cap > 0 && (!o.kp || !o.desc))) return fail(c, SPVO_ERR_INVALID, "bad output buffer");
    slots[0] = slot_l; slots[1] = slot_r;
    return SPVO_OK;
  }
  int check_capacity(int slot_capacity) {
    if (slot_capacity <= 0 || slot_capacity > F::CAP_MAX) return fail(c, SPVO_ERR_INVALID, "slot_capacity must be 1 .. %d", F::CAP_MAX);
    cap = slot_capacity;
    return SPVO_OK;
  }
  int open() {
    if (int rc = require_idle(c)) return rc;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    *out[0].n = *out[1].n = 0;
    return SPVO_OK;
  }
  int load(const uint8_t *img_l, const uint8_t *img_r, int rows, int cols, size_t stride) {
    PairStage &ps = F::pair(c);
    // both slots are being rewritten: whatever was matched against their old contents is stale
    for (int sl : slots) f.rewrite(c, sl);
    ps.mcache.invalidate();
    partner[0] = slots[1];
    partner[1] = ps.temporal_partner(slots[0], slots[1], ps.last_slot_l >= 0 && f.partner_ok(c, ps.last_slot_l));
    if (!F::FORGETS_AFTER_WAIT) ps.last_slot_l = -1;
    HIP_TRY(c, hipStreamSynchronize(c->stream2));   // (the staging buffer and the mirrors are the previous call's until its work is done)
    ps.stage(img_l, img_r, rows, cols, stride);
    px = (size_t)rows * cols;
    return F::before_chains(c);
  }
  const uint8_t *image(int k) const { return F::pair(c).h_img + k * px; }   // the staged image k (pinned, rows packed)
  // (a pair that turns out not to fit its slots is matched on whatever rows the slots hold; commit drops that result)
  int submit() {
    PairStage &ps = F::pair(c);
    HIP_TRY(c, hipEventRecord(ps.ev_feat, c->stream2));
    if (int rc = F::enqueue_prematch(c, slots[0], partner, cap)) return rc;
    HIP_TRY(c, wait_event(ps.ev_feat));   // the one wait of the call: the matches go on behind it
    if (F::FORGETS_AFTER_WAIT) ps.last_slot_l = -1;
    return SPVO_OK;
  }
  int count(int k) { return *out[k].n = F::h_n(c)[4 * k]; }
  int ncopy(int k) const { return std::min(*out[k].n, out[k].cap); }
  int commit(const PairMirror m[2]) {
    if (*out[0].n > cap || *out[1].n > cap) return fail(c, SPVO_ERR_CAPACITY, "%s: %d / %d rows do not fit slots of %d (slot_capacity)", who, *out[0].n, *out[1].n, cap);
    for (int k = 0; k < 2; ++k) {
      SlotState &s = F::slot(c, slots[k]);
      s.n = *out[k].n; s.filled = true;
      const int n = ncopy(k);
      if (n > 0 && out[k].kp && m[k].kp) std::memcpy(out[k].kp, m[k].kp, (size_t)n * m[k].kp_bytes);
      if (n > 0 && out[k].desc) std::memcpy(out[k].desc, m[k].desc, (size_t)n * m[k].row_bytes);
    }
    F::record_prematch(c, slots[0], partner, cap);
    F::pair(c).last_slot_l = slots[0];
    return SPVO_OK;
  }
};

// the binary slots (spvo_ctx::bin): rows of `row_bytes`, matched by enqueue_binary_prematch (Hamming, or byte-L2 under SPVO_NORM_L2) on the solver's stream, results in h_match + k * cap
struct BinPairFamily {
  int row_bytes;
  static constexpr int SLOTS = N_BIN_SLOTS, CAP_MAX = 1 << HAM_KEY_SHIFT;
  static constexpr bool OUT_NEEDS_BUFFERS = false, FORGETS_AFTER_WAIT = true;
  static PairStage &pair(spvo_ctx *c) { return c->bin.pair; }
  static const int *h_n(spvo_ctx *c) { return c->bin.h_n; }
  static SlotState &slot(spvo_ctx *c, int i) { return c->bin.slots[i]; }
  void rewrite(spvo_ctx *c, int i) const { slot_rewrite(c->bin.slots[i]); c->bin.slots[i].row_bytes = row_bytes; }
  // any filled slot of the same row width is a temporal partner, whichever entry point filled it; a slot of another width is skipped
  bool partner_ok(spvo_ctx *c, int prev) const { return c->bin.slots[prev].filled && c->bin.slots[prev].row_bytes == row_bytes; }
  static int before_chains(spvo_ctx *) { return SPVO_OK; }
  // counts read on the device; the matches run on the chains' stream, so ev_match is recorded there and nothing waits across streams
  static int enqueue_prematch(spvo_ctx *c, int slot_l, const int partner[2], int cap) {
    if (!c->prematch) return SPVO_OK;
    for (int k = 0; k < 2; ++k)
      if (partner[k] >= 0)
        if (int rc = enqueue_binary_prematch(c, slot_l, partner[k], c->bin.h_match + (size_t)k * cap)) return rc;
    HIP_TRY(c, hipEventRecord(c->bin.pair.ev_match, c->stream2));
    return SPVO_OK;
  }
  static void record_prematch(spvo_ctx *c, int slot_l, const int partner[2], int cap) {
    if (!c->prematch) return;
    auto &bb = c->bin;
    for (int k = 0; k < 2; ++k)
      if (partner[k] >= 0)
        bb.pair.mcache.record(k, slot_l, partner[k], bb.slots[slot_l].gen, bb.slots[partner[k]].gen, c->pm_selector, c->pm_cross, c->pm_ratio, bb.h_match + (size_t)k * cap, c->bin_pm_norm);
  }
};

}  // namespace spvo_int
#pragma GCC visibility pop
