#!/usr/bin/env python3
"""Static SALU / VALU / memory instructions of sb_block_kernel<WIDE> per source region of swz_mdblock.hip (offline: no GPU needed).
The listing must carry line tables:
  hipcc --offload-arch=gfx950 <the Makefile's flags> -gline-tables-only --cuda-device-only -S swz_mdblock.hip -o mdblock.s
usage: isa_regions.py mdblock.s swz_mdblock.hip [0|1]     (0: the narrow kernel, the default; 1: the wide one)
The totals equal tools/isa_count.py's on a listing without line tables."""
import os, re, sys
out, src = sys.argv[1], sys.argv[2]
kernel = '_ZN3swz15sb_block_kernelILb%sE' % (sys.argv[3] if len(sys.argv) > 3 else '0')
lines = open(src).read().split('\n')
def find(pat, start=0):
    for i in range(start, len(lines)):
        if pat in lines[i]: return i + 1
    raise KeyError(pat)
marks = [
 ('helpers (expand3, loads)', find('sb_expand3(uint32_t v)')),
 ('staging: points, region cell', find('sb_pack(uint32_t x')),
 ('exact compare', find('sb_exact_near(const SbArgs')),
 ('staging: points, region cell ', find('struct SbBlock')),
 ('staging: halo slot', find('sb_halo_slot(const SbLds')),
 ('masks: earlier', find('sb_earlier_mask(uint32_t ix')),
 ('masks: occupancy + reach', find('struct SbOwn')),
 ('search', find('sb_compare(const SbArgs')),
 ('state lookup', find('sb_state_of(const SbArgs')),
 ('kernel: prologue + ticket', find('void sb_block_kernel(SbArgs a)')),
 ('kernel: granules', find('---- the granules of the block')),
 ('staging: loop', find('---- stage the points')),
 ('cell index', find('---- the cell index of the region')),
 ('search: rounds, pending pairs', find('---- from here on every wavefront')),
 ('decisions: first look', find("// The neighbours' states as far as they are known now")),
 ('decisions: passes', find('// decisions: passes over the wavefront')),
 ('tail', find('SB_T(5);')),
 ('END', find('// ----------------------------------------------------------------------------- the granule table')),
]
marks.sort(key=lambda m: m[1])
def region(ln):
    r = None
    for name, start in marks:
        if ln >= start: r = name
    return r
s = open(out).read().split('\n')
files = {}
cnt = {}
inside = False
cur = ('other', 0)
for l in s:
    m = re.match(r'\s*\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', l)
    if m: files[int(m.group(1))] = (m.group(3) or m.group(2))
    if l.startswith(kernel): inside = True
    if inside and l.startswith('.Lfunc_end'): inside = False
    m = re.match(r'\s*\.loc\s+(\d+)\s+(\d+)', l)
    if m:
        f = files.get(int(m.group(1)), '')
        cur = (os.path.basename(f), int(m.group(2)))
    t = l.strip()
    if inside and t and not t.startswith(('.', ';')) and not t.endswith(':'):
        op = t.split()[0]
        if cur[0] == os.path.basename(src): r = (region(cur[1]) or "helpers (expand3, loads)").strip()
        elif cur[0] == 'swz_scan.h' or cur[0] == 'swz_device.h': r = 'kernel: granules' if 'scan' in cur[0] else 'staging: points, region cell'
        else: r = 'other (' + cur[0] + ')'
        c = cnt.setdefault(r, [0, 0, 0])
        if op.startswith('s_'): c[0] += 1
        elif op.startswith('v_'): c[1] += 1
        else: c[2] += 1
tot = [0,0,0]
for r, c in sorted(cnt.items()):
    print('%-34s SALU %5d  VALU %5d  mem %4d' % (r, *c))
    tot = [a+b for a,b in zip(tot,c)]
print('%-34s SALU %5d  VALU %5d  mem %4d' % ('TOTAL', *tot))
