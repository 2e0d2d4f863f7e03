#!/usr/bin/env python
"""SGPR spill moves of the kernels in gfx950 assembly files (the *-gfx950.s that the Makefile's -save-temps leaves under csrc/build/<unit>/).

An SGPR that does not fit is kept in a lane of a VGPR: v_writelane_b32 spills it, v_readlane_b32 brings it back, and each is a vector-ALU issue slot.
Per kernel: the static count of both, and how many of the reads lie inside the step loop as opposed to the prologue and the item loop around it.
A spill VGPR is one that some v_writelane_b32 of the kernel writes (the sources have no writelane builtin; the readlane builtins of the schedule read
VGPRs no writelane touches, and are not counted).  The step loop of a persistent kernel (persist_loop's loop over the steps of a run) is the loop of
depth 2 that holds the most instructions -- the loop nest is read from the compiler's own block comments ("in Loop: Header=.. Depth=..",
"Parent Loop .."); a kernel without a loop of depth 2 has no such column.

  python tools/spill_moves.py cage_challenge_4_amd/csrc/build/*/*-gfx950.s  [> profiles/rNN_spill_moves.txt]
"""
import re
import sys

LABEL = re.compile(r'^(\.LBB\d+_\d+):')
FUNC = re.compile(r'^([A-Za-z_][\w$.]*):\s*; @')
IN_LOOP = re.compile(r'in Loop: Header=(BB\d+_\d+) Depth=(\d+)')
PARENT = re.compile(r'Parent Loop (BB\d+_\d+) Depth=(\d+)')
HEADER = re.compile(r'This (?:Inner )?Loop Header: Depth=(\d+)')
WRITE = re.compile(r'^\s+v_writelane_b32\s+(v\d+),')
READ = re.compile(r'^\s+v_readlane_b32\s+s\d+,\s*(v\d+),')
INSN = re.compile(r'^\s+[a-z]\w+')


def kernels(lines):
    """(name, lines) of every function of the file"""
    name, body = None, []
    for ln in lines:
        m = FUNC.match(ln)
        if m:
            name, body = m.group(1), []
        elif name and ln.startswith('.Lfunc_end'):
            yield name, body
            name = None
        elif name:
            body.append(ln)


def scan(body):
    """per instruction: (text, innermost loop header or None); the parents and depth of every loop header"""
    parents, depth = {}, {}
    out = []
    cur = None                      # innermost loop of the current block
    label, pend_parents = None, []
    for ln in body:
        m = LABEL.match(ln)
        if m or ln.startswith('; %bb.'):
            label = m.group(1)[2:] if m else None
            cur, pend_parents = None, []
        for p in PARENT.finditer(ln):
            pend_parents.append(p.group(1))
        h = HEADER.search(ln)
        if h and label:
            parents[label] = list(pend_parents)
            depth[label] = int(h.group(1))
            cur = label
        il = IN_LOOP.search(ln)
        if il:
            cur = il.group(1)
        if INSN.match(ln) and not ln.lstrip().startswith(';'):
            out.append((ln, cur))
    return out, parents, depth


def report(name, body):
    insns, parents, depth = scan(body)
    spill_regs = {m.group(1) for ln, _ in insns for m in [WRITE.match(ln)] if m}
    def chain(h):
        return [] if h is None else [h] + parents.get(h, [])
    size = {}
    for _, h in insns:
        for a in chain(h):
            if depth.get(a) == 2:
                size[a] = size.get(a, 0) + 1
    step = max(size, key=size.get) if size else None
    writes = sum(1 for ln, _ in insns if WRITE.match(ln))
    reads = in_step = 0
    for ln, h in insns:
        m = READ.match(ln)
        if m and m.group(1) in spill_regs:
            reads += 1
            if step and step in chain(h):
                in_step += 1
    return (f'{name:52s} instructions {len(insns):6d}  spill_writes {writes:4d}  spill_reads {reads:4d}  '
            f'reads_in_step_loop {in_step if step else "-":>4}  step_loop {step or "-"} ({size.get(step, 0)} instructions)')


def main():
    rows = []
    for path in sys.argv[1:]:
        for name, body in kernels(open(path).read().splitlines()):
            rows.append(report(name, body))
    print('# SGPR spill moves per kernel (tools/spill_moves.py): v_writelane_b32 / v_readlane_b32 on spill VGPRs, static counts')
    for r in sorted(rows):
        print(r)


if __name__ == '__main__':
    main()
