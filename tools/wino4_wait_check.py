"""By-hand check of conv_wino4_kernel's items with counted operand waits (conv_wino4.hip.h, ITEM = 1 and ITEM = 2) on their compiled assembly.

The item issues its operand reads in inline assembly, which the compiler does not track: it believes the destination registers are
written when the asm statement ends.  Two things could go wrong after a change of WINO4_ITEM_LEAD, of the H1 / H2 slots or of the
compiler: a wait counted too short, or an instruction the compiler places between a read and its wait that touches the destination
(a copy, a spill).  This script replays one kernel's listing in textual order with the in-order LDS queue holding ONLY the inline-asm
reads -- the fewest that can be outstanding; every LDS operation the compiler adds makes the true count larger -- and reports any
instruction that reads or writes a register whose read has not been waited for, and any read whose destination overlaps a pending one.
With a second argument the role-conditional reads of the transform (those through the address register of a ds_read2_b32) are left
out as well: the other role's path.  Per item (barrier to barrier) it prints the instruction mix and the lgkmcnt waits between the
first and the last matrix instruction.

ITEM = 2 differs from ITEM = 1 in the form of its LDS-DMA only, and that stays the compiler's builtin (the scalar-base form is
reached by keeping the operands opaque, not by assembly), so the compiler still counts vmcnt and still owns M0.  Per item the script
counts the DMA that kept a vector address (a 64-bit vector add in front of each): 0 in an ITEM = 2 listing, all 7 in an ITEM = 1
listing.  Inline assembly that is no read (experiments have had the transform's arithmetic and its ds_write_b32 there) only READS
registers the compiler knows to be written; it is checked like any compiler instruction -- it must not touch a pending read's
destination -- and asm stores, which lengthen the LDS queue and so only make a counted wait safer, are counted apart ("lds_asm_store").

  hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S csrc/spvo_net_f32.hip -o net_f32.s
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


def main():
    path = sys.argv[1]
    other_role = len(sys.argv) > 2
    text = open(path).read()
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
    print("LDS-DMA in the kernel:", ", ".join(f"{v} with {k}" for k, v in dma_forms.items()))
    print("hazards:", bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
