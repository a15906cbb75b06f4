#!/usr/bin/env python3
"""Register copies in the loops of one kernel, from `hipcc -S --cuda-device-only
-gline-tables-only` output (gfx950).

Prints, for every loop-header block (the blocks the compiler's own listing
comments mark "Loop Header") and for every run of four or more consecutive copies (`v_mov_b32`,
`s_mov_b32`, `s_mov_b64`; waits and `s_nop` do not end a run):
the block label, the nearest source line, and the `v_mov` / `s_mov` counts;
then the kernel's totals: instructions, SALU, VALU, branches, `v_mov`, `s_mov`,
exec-mask regions (`s_*_saveexec_b64`), VGPRs, SGPR spills, scratch bytes.
VALU counts every `v_` mnemonic (`v_cmp`, `v_readlane`, `v_readfirstlane` too);
SALU every `s_` one but branches, waits, `s_nop`, scalar loads and the like.

usage: sim_copies.py file.s 'kernel name regex' [--all]   (--all: every kernel
that matches, totals only, one line each: the table of all builds)

  hipcc <the Makefile's flags for sim_wave.hip> -S --cuda-device-only \\
      -gline-tables-only -o sim_wave.s fantoch_amd/csrc/sim_wave.hip
  python3 tools/sim_copies.py sim_wave.s 'k_simILj1ELj1ELj4ELj1ENS0_5GeoCT'"""
import re
import sys

NOT_SALU = ("s_branch", "s_cbranch", "s_setpc", "s_swappc", "s_call", "s_waitcnt", "s_nop", "s_endpgm", "s_barrier",
            "s_load", "s_buffer_load", "s_mem", "s_sleep", "s_setprio", "s_sendmsg", "s_code_end", "s_trap",
            "s_inst_prefetch", "s_icache", "s_set_gpr_idx")
BRANCH = ("s_branch", "s_cbranch", "s_setpc", "s_swappc", "s_call")
TRANSPARENT = ("s_waitcnt", "s_nop")  # do not end a run of copies


def kernels(path, pattern):
    """name -> (body lines, trailer lines up to the next symbol)"""
    out, name, body, trailer, in_body = {}, None, [], [], False
    for line in open(path):
        m = re.match(r"^(\w+):\s*(;.*)?$", line)
        if m and not line.startswith(".L"):
            if name:
                out[name] = (body, trailer)
            hit = re.search(pattern, m.group(1)) and not m.group(1).endswith(".kd")
            name, body, trailer, in_body = (m.group(1) if hit else None), [], [], True
            continue
        if name is None:
            continue
        if in_body and re.match(r"^\s*s_endpgm", line):
            body.append(line)
            continue
        if in_body and (line.startswith("\t.section") or line.startswith(".Lfunc_end")):
            in_body = False
        (body if in_body else trailer).append(line)
    if name:
        out[name] = (body, trailer)
    return out


def mnemonic(line):
    code = line.split(";")[0].strip()
    if not code or code.startswith(".") or code.endswith(":"):
        return None
    return code.split()[0]


def is_vmov(m):
    return m.startswith("v_mov_b32")


def is_smov(m):
    return m in ("s_mov_b32", "s_mov_b64")


def analyse(body, trailer):
    # instructions with their block and the last .loc line before them
    insts, labels, block, line_no = [], {}, "(entry)", 0
    block_note, at_label = {}, False
    for raw in body:
        m = re.match(r"^(\.LBB\d+_\d+):\s*(;.*)?$", raw)
        if m:
            block = m.group(1)
            labels[block] = len(insts)
            block_note[block] = (m.group(2) or "").strip("; \n")
            at_label = True
            continue
        if at_label and re.match(r"^\s*;", raw):  # the label's comment goes on over several lines
            block_note[block] += " | " + " ".join(raw.strip("; \n").split())
            continue
        at_label = False
        m = re.match(r"^\s*\.loc\s+\d+\s+(\d+)", raw)
        if m:
            line_no = int(m.group(1))
            continue
        mn = mnemonic(raw)
        if mn is None:
            continue
        tgt = None
        if mn.startswith(BRANCH):
            t = re.search(r"(\.LBB\d+_\d+)", raw)
            tgt = t.group(1) if t else None
        insts.append((mn, block, line_no, tgt))
    headers = {b for b, note in block_note.items() if "Loop Header" in note}
    tot = dict(instructions=len(insts), salu=0, valu=0, branches=0, v_mov=0, s_mov=0, exec_regions=0)
    per_block = {}
    for mn, blk, ln, _ in insts:
        b = per_block.setdefault(blk, dict(n=0, v=0, s=0, line=ln))
        b["n"] += 1
        if mn.startswith("v_"):
            tot["valu"] += 1
        if mn.startswith(BRANCH):
            tot["branches"] += 1
        elif mn.startswith("s_") and not mn.startswith(NOT_SALU):
            tot["salu"] += 1
        if is_vmov(mn):
            tot["v_mov"] += 1
            b["v"] += 1
        if is_smov(mn):
            tot["s_mov"] += 1
            b["s"] += 1
        if re.match(r"s_\w+_saveexec_b64", mn):
            tot["exec_regions"] += 1
    # runs of >= 4 consecutive copies
    runs, cur = [], None
    for mn, blk, ln, _ in insts:
        if is_vmov(mn) or is_smov(mn):
            if cur is None or cur["block"] != blk:
                if cur and cur["v"] + cur["s"] >= 4:
                    runs.append(cur)
                cur = dict(block=blk, line=ln, v=0, s=0)
            cur["v" if is_vmov(mn) else "s"] += 1
        elif mn.startswith(TRANSPARENT):
            continue
        else:
            if cur and cur["v"] + cur["s"] >= 4:
                runs.append(cur)
            cur = None
    if cur and cur["v"] + cur["s"] >= 4:
        runs.append(cur)
    text = "".join(trailer)

    def num(rx):
        m = re.search(rx, text)
        return int(m.group(1)) if m else None

    tot["vgprs"] = num(r";\s*NumVgprs:\s*(\d+)")
    tot["sgpr_spills"] = num(r";\s*SGPRSpill:\s*(\d+)") if "SGPRSpill" in text else None
    tot["scratch"] = num(r";\s*ScratchSize:\s*(\d+)")
    return tot, headers, per_block, block_note, runs


def spills_from_metadata(path, name):
    """.sgpr_spill_count / .vgpr_spill_count of `name` in the file's metadata"""
    text = open(path).read()
    m = re.search(r"^\s+\.name:\s+%s\s*$" % re.escape(name), text, re.M)
    if not m:
        return None, None
    rest = text[m.end():]  # the entry's keys are in alphabetical order: both counts follow the name
    s = re.search(r"\.sgpr_spill_count:\s+(\d+)", rest)
    v = re.search(r"\.vgpr_spill_count:\s+(\d+)", rest)
    return (int(s.group(1)) if s else None), (int(v.group(1)) if v else None)


def main():
    if len(sys.argv) < 3:
        print(__doc__)
        return 2
    path, pattern = sys.argv[1], sys.argv[2]
    every = "--all" in sys.argv[3:]
    ks = kernels(path, pattern)
    if not ks:
        print("no kernel matches %r" % pattern)
        return 1
    if not every and len(ks) > 1:
        print("%d kernels match %r:" % (len(ks), pattern))
        for k in sorted(ks):
            print("  " + k)
        return 1
    for name in sorted(ks):
        tot, headers, per_block, note, runs = analyse(*ks[name])
        ss, vs = spills_from_metadata(path, name)
        if tot["sgpr_spills"] is None:
            tot["sgpr_spills"] = ss
        tot["vgpr_spills"] = vs
        if every:
            print("%s\n    insts %d  v_mov %d  s_mov %d  VGPRs %s  SGPR spills %s  VGPR spills %s  scratch %s" % (
                name, tot["instructions"], tot["v_mov"], tot["s_mov"], tot["vgprs"], tot["sgpr_spills"],
                tot["vgpr_spills"], tot["scratch"]))
            continue
        print(name)
        print("loop-header blocks (label, source line, instructions, v_mov, s_mov, note):")
        order = [b for b in per_block if b in headers]
        for b in order:
            d = per_block[b]
            print("  %-12s line %-5d %4d insts  %3d v_mov  %3d s_mov  %s" % (b, d["line"], d["n"], d["v"], d["s"],
                                                                         note.get(b, "")))
        print("  total in loop headers: %d v_mov, %d s_mov" % (sum(per_block[b]["v"] for b in order),
                                                             sum(per_block[b]["s"] for b in order)))
        print("runs of >= 4 consecutive copies (block, source line, v_mov, s_mov):")
        for r in runs:
            print("  %-12s line %-5d %3d v_mov  %3d s_mov%s" % (r["block"], r["line"], r["v"], r["s"],
                                                              "  (loop header)" if r["block"] in headers else ""))
        print("  total in runs: %d v_mov, %d s_mov in %d runs" % (sum(r["v"] for r in runs), sum(r["s"] for r in runs),
                                                                len(runs)))
        print("totals: " + "  ".join("%s %s" % (k, v) for k, v in tot.items()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
