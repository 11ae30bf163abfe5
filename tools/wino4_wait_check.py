"""By-hand check of conv_wino4_kernel's items with counted operand waits (conv_wino4.hip.h, ITEM = 1, 2 and 3) on their compiled assembly.

The item issues its operand reads in inline assembly, which the compiler does not track: it believes the destination registers are
written when the asm statement ends.  Two things could go wrong after a change of WINO4_ITEM_LEAD, of the H1 / H2 slots or of the
compiler: a wait counted too short, or an instruction the compiler places between a read and its wait that touches the destination
(a copy, a spill).  This script replays one kernel's listing in textual order with the in-order LDS queue holding ONLY the inline-asm
reads -- the fewest that can be outstanding; every LDS operation the compiler adds makes the true count larger -- and reports any
instruction that reads or writes a register whose read has not been waited for, and any read whose destination overlaps a pending one.
With a second argument the role-conditional reads of the transform (those through the address register of a ds_read2_b32) are left
out as well: the other role's path.  Per item (barrier to barrier) it prints the instruction mix and the lgkmcnt waits between the
first and the last matrix instruction, and the dynamic instruction count of the steady-state item by class (hot_path below).  Given the
listing of a whole unit it checks every conv_wino4_kernel in it.

ITEM = 2 differs from ITEM = 1 in the form of its LDS-DMA only, and that stays the compiler's builtin (the scalar-base form is
reached by keeping the operands opaque, not by assembly), so the compiler still counts vmcnt and still owns M0.  Per item the script
counts the DMA that kept a vector address (a 64-bit vector add in front of each): 0 in an ITEM = 2 listing, all 7 in an ITEM = 1
listing.  Inline assembly that is no read (experiments have had the transform's arithmetic and its ds_write_b32 there) only READS
registers the compiler knows to be written; it is checked like any compiler instruction -- it must not touch a pending read's
destination -- and asm stores, which lengthen the LDS queue and so only make a counted wait safer, are counted apart ("lds_asm_store").

ITEM = 3 has its counted operand waits with the pieces as inputs only, so nothing but the order of the listing puts a wait in front of
its matrix instruction: this replay is the check of that order (a matrix instruction that moved in front of its wait touches a
pending destination), to be run on every library instance in both roles after a change of the item or of the compiler.

  hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S csrc/spvo_net_f32.hip -o net_f32.s
  python tools/wino4_wait_check.py net_f32.s && python tools/wino4_wait_check.py net_f32.s other-role      (every instance in the unit), or one kernel:
  awk '/^_ZN4spvo17conv_wino4_kernelILb1ELb1ELi1ELi2ELi2EEEvNS_8ConvArgsE:/,/^\\.Lfunc_end/' net_f32.s > k.s     (ITEM = 1: ...ELi2ELi1EEE...)
  python tools/wino4_wait_check.py k.s && python tools/wino4_wait_check.py k.s other-role
"""
import re
import sys


def regs(text):
    out = set()
    for m in re.finditer(r"\bv\[(\d+):(\d+)\]", text):
        out.update(range(int(m.group(1)), int(m.group(2)) + 1))
    for m in re.finditer(r"\bv(\d+)\b", text):
        out.add(int(m.group(1)))
    return out


def hot_path(text, role):
    """Dynamic instruction count of the steady-state item by class: one walk through the depth-2 item loop (the body with 36 matrix
    instructions) from its header back to its header, for a wave in the given role (True: the first half of a transform, False: the
    second).  Branches: a test of a scalar against the literal 0 is the role test (the item has no other) and goes the role's way; every
    other conditional branch is taken when it goes backwards (the loop's back edge) or when the block it jumps over holds an integer division
    (decode(): the once-per-tile blocks, left out), and not taken otherwise -- a wave whose cursors stay inside their tile, that has
    tiles left to stage, and that carries all seven DMA pieces.  s_waitcnt and s_nop are counted apart from the other scalar instructions."""
    lines = text.splitlines()
    labels = {}
    for i, line in enumerate(lines):
        m = re.match(r"(\.LBB\d+_\d+):", line)
        if m:
            labels[m.group(1)] = i
    out = []
    for lab, start in labels.items():
        if "Depth=2" not in " ".join(lines[start:start + 2]) or "Inner Loop Header" not in " ".join(lines[start:start + 2]):
            continue
        cnt = dict(mfma=0, valu=0, lds=0, dma=0, scalar=0, s_nop=0, waits=0)
        i, scc, steps = start + 1, None, 0
        while steps < 20000:
            steps += 1
            if i >= len(lines):
                break
            if i == start:
                break
            t = lines[i].split(";")[0].strip()
            i += 1
            if not t or t.endswith(":") or t.startswith("."):
                continue
            op = t.split()[0]
            if op.startswith("v_mfma"):
                cnt["mfma"] += 1
            elif op.startswith("global_load_lds"):
                cnt["dma"] += 1
            elif op.startswith("ds_"):
                cnt["lds"] += 1
            elif op.startswith("v_"):
                cnt["valu"] += 1
            elif op == "s_nop":
                cnt["s_nop"] += 1
            elif op == "s_waitcnt":
                cnt["waits"] += 1
            elif op.startswith("s_"):
                cnt["scalar"] += 1
            m = re.match(r"s_cmp_(eq|lg)_u32 s\d+, 0$", t)
            if m:
                scc = (not role) if m.group(1) == "eq" else role   # role scalar != 0 in the first-half role
            elif op.startswith("s_cmp") or op.startswith("s_bitcmp"):
                scc = None
            if op == "s_branch":
                i = labels[t.split()[1]]
            elif op.startswith("s_cbranch"):
                tgt = labels[t.split()[1]]
                if op in ("s_cbranch_scc0", "s_cbranch_scc1") and scc is not None:
                    taken = scc == (op == "s_cbranch_scc1")
                else:   # backwards: the back edge; forwards over a block with an integer division (decode()): the once-per-tile block, skipped
                    nxt = next((j for j in range(i, len(lines)) if re.match(r"\.LBB\d+_\d+:", lines[j])), len(lines))
                    taken = tgt < i or any(x.split(";")[0].strip().startswith("s_abs_i32") for x in lines[i:nxt])
                if taken:
                    i = tgt
        if cnt["mfma"] == 36:
            out.append((start + 1, cnt))
    return out


def main():
    path = sys.argv[1]
    other_role = len(sys.argv) > 2
    whole = open(path).read()
    # a listing of a whole unit: every conv_wino4_kernel in it, one after the other
    parts = re.findall(r"^(_ZN4spvo17conv_wino4_kernel\w+):[^\n]*\n(.*?)^\.Lfunc_end", whole, re.S | re.M)
    if not parts:
        return check(whole, other_role)
    rc = 0
    for name, text in parts:
        print(name)
        rc |= check(name + ":\n" + text, other_role)
    return rc


def check(text, other_role):
    xf_addr = set(re.findall(r"ds_read2_b32 v\[\d+:\d+\], (v\d+)", text))
    in_asm, queue, bad, items, cur = False, [], 0, [], None
    dma_forms = {"scalar base": 0, "vector address": 0}
    for i, line in enumerate(text.splitlines()):
        t = line.strip()
        if t.startswith(";;#ASMSTART"):
            in_asm = True
            continue
        if t.startswith(";;#ASMEND"):
            in_asm = False
            continue
        if not t or t[0] in ";." or t.endswith(":"):
            continue
        t = t.split(";")[0].strip()
        op = t.split()[0]
        if op.startswith("global_load_lds"):
            dma_forms["scalar base" if re.search(r",\s*s\[\d+:\d+\]", t) else "vector address"] += 1
            if cur is not None:
                cur["lds_dma_vector_address"] += 0 if re.search(r",\s*s\[\d+:\d+\]", t) else 1
        if op == "s_barrier":
            if cur:
                items.append(cur)
            cur = dict(line=i + 1, mfma=0, valu=0, salu=0, branch=0, lds_asm=0, lds_asm_store=0, lds_compiler=0, lds_dma=0, lds_dma_vector_address=0, waits=[])
            continue
        if cur is None:
            continue
        if op == "s_waitcnt":
            m = re.search(r"lgkmcnt\((\d+)\)", t)
            if m:
                n = int(m.group(1))
                del queue[:max(0, len(queue) - n)]
                if 0 < cur["mfma"] < 36:
                    cur["waits"].append((n, "asm" if in_asm else "compiler"))
            continue
        if in_asm and op.startswith("ds_read"):
            if other_role and t.split(",")[1].split()[0] in xf_addr:
                continue
            dst = regs(t.split(",")[0])
            if any(q & dst for q in queue):
                print(f"line {i + 1}: destination overlaps a pending read: {t}")
                bad += 1
            queue.append(dst)
            cur["lds_asm"] += 1
            continue
        touched = regs(t)
        for q in queue:
            if q & touched:
                print(f"line {i + 1}: touches pending v{sorted(q & touched)}: {t}")
                bad += 1
        if op.startswith("v_mfma"):
            cur["mfma"] += 1
        elif op.startswith("ds_"):
            cur["lds_asm_store" if in_asm else "lds_compiler"] += 1
        elif op.startswith("global_load_lds"):
            cur["lds_dma"] += 1
        elif op.startswith("v_"):
            cur["valu"] += 1
        elif op.startswith(("s_cbranch", "s_branch")):
            cur["branch"] += 1
        elif op.startswith("s_"):
            cur["salu"] += 1
    if cur:
        items.append(cur)
    for it in items:
        if it["mfma"] == 36:
            full = sum(1 for n, who in it["waits"] if n == 0)
            print(f"item at line {it['line']}: " + ", ".join(f"{k} {it[k]}" for k in ("valu", "salu", "branch", "lds_asm", "lds_asm_store", "lds_compiler", "lds_dma", "lds_dma_vector_address"))
                  + f"; lgkmcnt waits inside: {len(it['waits'])}, of which lgkmcnt(0): {full}, placed by the compiler: {sum(1 for _, w in it['waits'] if w == 'compiler')}")
    for line, cnt in hot_path(text, not other_role):
        print(f"hot path of the item loop at line {line}, {'second' if other_role else 'first'}-half role: " + ", ".join(f"{k} {v}" for k, v in cnt.items()) + f"; total {sum(cnt.values())}")
    print("LDS-DMA in the kernel:", ", ".join(f"{v} with {k}" for k, v in dma_forms.items()))
    print("hazards:", bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
