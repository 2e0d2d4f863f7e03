#!/usr/bin/env python
"""LDS traffic on the red agents' headers and on the action records, in gfx950 assembly files (the *-gfx950.s that the Makefile's -save-temps leaves
under csrc/build/<unit>/): which ds_read / ds_write instructions of a kernel address RedHdr (RedAgent.h), EnvState.rexec / bexec or BlueAgent.queue,
and how wide each is.

The one-wave kernels address the staged row as base register + literal offset, the literal being the offset in the row (an agent's lane adds
r * sizeof(RedAgent) in the register), so an instruction belongs to a region when its literal offset falls into it -- for a per-agent region, into the
copy of any agent.  The regions come from the offsets the oracle prints (cc4o_layout: oracle/liboracle.so, built by `make -C oracle`).  ds_read2 /
ds_write2 count once per address.  A field the oracle's listing does not name shows as the named field in front of it + k (nlive = nobs+1, rsc_dirty =
start_host+1).  Not seen: an access whose address is all in the register (offset 0), or whose register is indexed by something else than the agent's
number (blue agent b on lane 8 + b: the literal is 64 short).  Static counts, not executions.

  python tools/hdr_traffic.py [--kernel NAME_PART] cage_challenge_4_amd/csrc/build/cc4_k_run1/*-gfx950.s  [> profiles/rNN_hdr_traffic.txt]
"""
import ctypes
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNC = re.compile(r'^([A-Za-z_][\w$.]*):\s*; @')
DS = re.compile(r'^\s+(ds_(?:read|write)\w*)\s+(.*)$')
OFFS = re.compile(r'offset([01]?):(\d+)')
WIDTH = {'u8': 1, 'i8': 1, 'b8': 1, 'u16': 2, 'i16': 2, 'b16': 2, 'b32': 4, 'b64': 8, 'b96': 12, 'b128': 16}
NRED, NBLUE, HDR, ACT = 6, 5, 32, 8


def layout():
    lib = ctypes.CDLL(os.path.join(ROOT, 'oracle', 'liboracle.so'))
    buf = ctypes.create_string_buffer(8192)
    n = lib.cc4o_layout(buf, 8192)
    return {k: int(v) for k, v in (ln.split() for ln in buf.raw[:n].decode().splitlines())}


def regions(L):
    """[(name, first byte, bytes, {offset in the region: field name})]"""
    hdr0 = L['red.queue']
    fields = {v - hdr0: k[4:] for k, v in L.items() if k.startswith('red.') and hdr0 <= v < hdr0 + HDR}
    out = []
    for r in range(NRED):
        out.append(('RedHdr', L['red'] + r * L['sizeof.RedAgent'] + hdr0, HDR, fields))
    out.append(('rexec', L['rexec'], NRED * ACT, None))
    out.append(('bexec', L['bexec'], NBLUE * ACT, None))
    for b in range(NBLUE):
        out.append(('BlueAgent.queue', L['blue'] + b * L['sizeof.BlueAgent'] + L['blue.queue'], ACT, None))
    return out


ACT_FIELDS = {0: 'type', 1: 'host', 2: 'arg', 3: 'ticks', 4: 'sid', 6: 'busy'}


def field_name(region, rel, fields):
    if fields is None:
        rel %= ACT
        fields = ACT_FIELDS
    base = max(k for k in fields if k <= rel)
    return f'{fields[base]}' + (f'+{rel - base}' if rel != base else '')


def accesses(line):
    """(mnemonic, width in bytes, [byte offsets]) of one ds_read / ds_write line, or None"""
    m = DS.match(line)
    if not m:
        return None
    op, rest = m.group(1), m.group(2).split(';')[0]
    ty = op.split('_')[-1]
    two = re.match(r'ds_(?:read|write)2(st64)?_', op)
    w = WIDTH.get(ty)
    if w is None:
        return None
    offs = {k: int(v) for k, v in OFFS.findall(rest)}
    if two:
        unit = w * (64 if two.group(1) else 1)
        return op, w, [offs.get('0', 0) * unit, offs.get('1', 0) * unit]
    return op, w, [offs.get('', 0)]


def kernels(lines):
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


def report(name, body, regs):
    rows, total = {}, {}
    for ln in body:
        a = accesses(ln)
        if not a:
            continue
        op, w, offs = a
        for off in offs:
            for rname, first, size, fields in regs:
                if first <= off < first + size:
                    rel = off - first
                    key = (rname, rel if fields is not None else rel % ACT, field_name(rname, rel, fields), op, w)
                    rows[key] = rows.get(key, 0) + 1
                    kind = 'read' if '_read' in op else 'write'
                    total[(rname, kind, w)] = total.get((rname, kind, w), 0) + 1
                    break
    out = [f'{name}']
    for (rname, rel, fname, op, w), cnt in sorted(rows.items()):
        out.append(f'  {rname:16s} +{rel:<3d} {fname:18s} {op:18s} {w:3d} B  x {cnt}')
    for rname in ('RedHdr', 'rexec', 'bexec', 'BlueAgent.queue'):
        for kind in ('read', 'write'):
            parts = [f'{cnt} x {w} B' for (rn, kd, w), cnt in sorted(total.items()) if rn == rname and kd == kind]
            n = sum(cnt for (rn, kd, w), cnt in total.items() if rn == rname and kd == kind)
            out.append(f'  total {rname:16s} {kind:5s} {n:4d} sites: ' + ', '.join(parts))
    return '\n'.join(out)


def main():
    args = sys.argv[1:]
    want = 'k_run_philox1'
    if args and args[0] == '--kernel':
        want, args = args[1], args[2:]
    regs = regions(layout())
    print('# LDS instructions on the red headers and the action records (tools/hdr_traffic.py): region, offset in the record, field, instruction, width, static sites')
    for path in args:
        for name, body in kernels(open(path).read().splitlines()):
            if want in name:
                print(report(name, body, regs))


if __name__ == '__main__':
    main()
