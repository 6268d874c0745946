"""The memory waits at the head and at the end of a tile of the three persistent inference kernels, counted in the COMPILED code
(profiles/r08_tile_front_waits.txt):

  python tools/tile_front_waits.py [--events] [asm of another build ...]

Without a file the current sources are compiled (hipcc -S --cuda-device-only with csrc/build.sh's flags, as tools/gen_isa_mix.py).
Per kernel, for the tile loop (tile_loop() below: the blocks of the loop around the MFMAs, in control-flow order from the loop's head):
  before the first gather load (k_attention_g has no gather: before its first MFMA) and between the last MFMA and the tile's last
  store: the EXPOSED round trips -- waits for a load that was issued with no MFMA in between, one per batch of loads -- and, apart,
  the waits for loads that have been in flight under at least one MFMA chain (the previous tile's network, or this tile's);
  head of the tile: the VMEM loads in front of the first gather load in issue order, with the waits between them.
A kernel that branches on the point mode inside the loop (the parent build) is counted over ALL its modes' blocks: an upper bound
for the ray-mode path.
VGPRs, scratch and occupancy come from the kernel's own resource directives.  --events prints every load / wait / store of the loop.
A kernel that takes the point mode as a template parameter is reported for its ray-mode instantiation (Lb1E)."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import bench                                                         # noqa: E402
import isa_mix                                                       # noqa: E402
from gen_isa_mix import FLAGS                                        # noqa: E402

KERNELS = ('k_decode_lc16I', 'k_decode_high_gI', 'k_attention_gI')


def pick(names, stem):
    c = [n for n in names if stem in n and 'train' not in n]
    ray = [n for n in c if 'Lb1E' in n]
    return (ray or c)[0]


def resources(path, name):
    text = open(path).read()
    i = text.index('.amdhsa_kernel ' + name)
    blk = text[i:text.index('.end_amdhsa_kernel', i)]
    vg = int(re.search(r'\.amdhsa_next_free_vgpr (\d+)', blk).group(1))
    acc = re.search(r'\.amdhsa_accum_offset (\d+)', blk)
    scratch = int(re.search(r'\.amdhsa_private_segment_fixed_size (\d+)', blk).group(1))
    arch = int(acc.group(1)) if acc else vg
    alloc = (vg + 7) // 8 * 8
    return arch, vg, scratch, min(8, 512 // alloc)


def tile_loop(body):
    """The tile loop as the control flow has it, not as the text has it (the block layout puts a loop's store block behind its
    back branch where it likes): the strongly connected blocks around the MFMAs, in reverse postorder from the loop's entry block
    with the back edges left out -- every path through a tile in ONE topological sequence (a count over it is an upper bound for
    any single path)."""
    starts = [0] + [i for i, l in enumerate(body) if re.match(r'^\.LBB\d+_\d+:', l)]
    starts = sorted(set(starts))
    label = {re.match(r'^(\.LBB\d+_\d+):', body[i]).group(1): k for k, i in enumerate(starts) if re.match(r'^\.LBB', body[i])}
    blocks = [body[a:b] for a, b in zip(starts, starts[1:] + [len(body)])]
    succ = []
    for k, blk in enumerate(blocks):
        s, fall = set(), True
        for l in blk:
            t = l.strip().split()
            if not t:
                continue
            m = re.search(r's_(cbranch_\w+|branch) (\.LBB\d+_\d+)', l)
            if m:
                s.add(label[m.group(2)])
                fall = m.group(1) != 'branch'
            elif t[0] == 's_endpgm':
                fall = False
            elif not t[0].startswith(('.', ';')) and not t[0].endswith(':'):
                fall = True
        if fall and k + 1 < len(blocks):
            s.add(k + 1)
        succ.append(s)
    mf = [k for k, blk in enumerate(blocks) if any(l.strip().startswith('v_mfma') for l in blk)]

    def reach(src, edges):
        seen, todo = set(), [src]
        while todo:
            x = todo.pop()
            for y in edges[x]:
                if y not in seen:
                    seen.add(y)
                    todo.append(y)
        return seen
    pred = [set() for _ in blocks]
    for k, s in enumerate(succ):
        for y in s:
            pred[y].add(k)
    scc = (reach(mf[0], succ) & reach(mf[0], pred)) | {mf[0]}
    heads = [k for k in sorted(scc) if any(x not in scc for x in pred[k])]
    head = heads[0]
    order, seen = [], set()

    def dfs(x):
        seen.add(x)
        for y in sorted(succ[x], reverse=True):
            if y in scc and y != head and y not in seen:
                dfs(y)
        order.append(x)
    sys.setrecursionlimit(10000)
    dfs(head)
    return [l for k in reversed(order) for l in blocks[k]]


def events(loop):
    ev = []
    for l in loop:
        t = l.strip().split()
        if not t or t[0].startswith(('.', ';')) or t[0].endswith(':'):
            continue
        op = t[0]
        if op.startswith('global_load') or op.startswith('buffer_load'):
            ev.append(('load', op))
        elif op.startswith('global_store') or op.startswith('buffer_store'):
            ev.append(('store', op))
        elif op.startswith('global_atomic'):
            ev.append(('atomic', op))
        elif op == 's_waitcnt' and 'vmcnt' in l:
            ev.append(('wait', re.search(r'vmcnt\((\d+)\)', l).group(1)))
        elif op.startswith('v_mfma'):
            ev.append(('mfma', op))
    return ev


def round_trips(ev):
    """ev over TWO iterations of the loop (a load issued in one tile and waited for in the next is seen with its issue point).  Every
    wait of the second iteration -> (index in ev, MFMAs executed between the issue of the youngest load it retires and the wait), or
    None for a wait that retires no load (nothing new, or stores only).  vmcnt counts loads, stores and returning atomics in order."""
    out, pending, nm = {}, [], 0
    n = len(ev)
    for i, e in enumerate(ev + ev):
        if e[0] == 'mfma':
            nm += 1
        elif e[0] in ('load', 'store', 'atomic'):
            pending.append((e[0], nm, i))
        elif e[0] == 'wait':
            keep = int(e[1])
            gone, pending = pending[:max(0, len(pending) - keep)], pending[max(0, len(pending) - keep):]
            loads = [g for g in gone if g[0] == 'load']
            if i >= n:
                out[i - n] = (nm - loads[-1][1], loads[-1][2] % n) if loads else None
    return out


def exposed(ev, trips, lo, hi):
    """Waits in ev[lo:hi] that pay a memory round trip: they retire a load issued with NO MFMA in between, and that load was issued
    after the previous such wait (vmcnt(1), vmcnt(0) on one batch of loads is one round trip).  Returns (exposed, covered)."""
    n_exp, n_cov, last = 0, 0, -1
    for i in range(lo, hi):
        t = trips.get(i)
        if ev[i][0] != 'wait' or t is None:
            continue
        if t[0] > 0:
            n_cov += 1
        elif t[1] > last or t[1] > i:        # (a load of the previous iteration's tail: index beyond the wait)
            n_exp += 1
            last = i
    return n_exp, n_cov


def report(path, show_events):
    ks = isa_mix.kernels(path)
    out = []
    for stem in KERNELS:
        name = pick(ks, stem)
        ev = events(tile_loop(ks[name]))
        is_g = [e == ('load', 'global_load_dwordx4') for e in ev]
        if 'attention' in stem:
            first = next(i for i, e in enumerate(ev) if e[0] == 'mfma')
        else:                                # the gather: the first run of four 16-byte loads (an explicit f64 point is one of them alone)
            first = next(i for i in range(len(ev)) if all(is_g[i:i + 4]) and len(is_g[i:i + 4]) == 4)
        last_mfma = max(i for i, e in enumerate(ev) if e[0] == 'mfma')
        last_store = max(i for i, e in enumerate(ev) if e[0] == 'store')
        trips = round_trips(ev)
        f_exp, f_cov = exposed(ev, trips, 0, first)
        e_exp, e_cov = exposed(ev, trips, last_mfma, last_store)
        arch, vg, scratch, occ = resources(path, name)
        what = 'MFMA' if 'attention' in stem else 'gather load'
        out.append(f'{name}\n    VGPRs {arch}, scratch {scratch} B, {occ} waves per SIMD\n'
                   f'    before the first {what}: {f_exp} exposed round trip(s), {f_cov} wait(s) for loads issued at least one MFMA chain earlier\n'
                   f'    between the last MFMA and the last store: {e_exp} exposed round trip(s), {e_cov} wait(s) for loads issued earlier in the tile\n'
                   f'    head of the tile: ' + ' '.join(e[1].replace('global_load_', '') if e[0] == 'load' else f'|vmcnt({e[1]})|'
                                                       for e in ev[:first] if e[0] in ('load', 'wait')))
        if show_events:
            run, prev = 0, None
            for e in ev + [None]:
                if e == prev:
                    run += 1
                    continue
                if prev is not None:
                    out.append(f'        {prev[0]} {prev[1]}' + (f' x {run}' if run > 1 else ''))
                prev, run = e, 1
    return '\n'.join(out)


def main():
    args = [a for a in sys.argv[1:] if a != '--events']
    show = '--events' in sys.argv
    print(f'# source_hash={bench.source_hash()}  tools/tile_front_waits.py: hipcc {" ".join(FLAGS)} -S --cuda-device-only')
    if not args:
        with tempfile.TemporaryDirectory() as d:
            asm = os.path.join(d, 'adfp.s')
            subprocess.check_call([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')] + FLAGS + ['-I' + os.path.join(ROOT, 'include'), '-S', '--cuda-device-only', '-o', asm,
                                   os.path.join(ROOT, 'attentive_dfprior_amd', 'csrc', 'adfp_kernels.hip')])
            print('== this build')
            print(report(asm, show))
    for a in args:
        print(f'== {os.path.basename(a)}')
        print(report(a, show))


if __name__ == '__main__':
    main()
