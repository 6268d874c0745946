"""The CPU table of DESIGN.md section 5.13.2: what the depth bilateral filter buys the depth ICP's float64 restatement
(tests/icp_ref.py, tests/depth_filter_ref.py) on the mini scene under sensor noise N(0, (s z^2)^2), s = 0.02, 0.03, 0.04 -- the 36
trials of tests/test_depth_filter_host.py per level -- and what it costs on clean depth.  No GPU.

    python tools/depth_filter_tally.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import depth_filter_ref as F                                   # noqa: E402
import icp_ref as R                                            # noqa: E402
from attentive_dfprior_amd import synthetic                    # noqa: E402


def main():
    sc = synthetic.mini_scene()
    intr = (sc.fx, sc.fy, sc.cx, sc.cy)
    cases = R.scene_cases(sc)
    sensor = {}
    base = []
    for ci in F.TALLY_CASES:
        P, G = cases[ci]
        if P.tobytes() not in sensor:
            sensor[P.tobytes()] = R.cpu_raycast(sc, P)
        base.append((ci, P, G, sensor[P.tobytes()], R.cpu_raycast(sc, G)))
    print('| noise s | input | status OK | translation error ≤ guess/3 | rotation error ≤ guess/2 | worst rotation error / guess | '
          'worst translation error / guess | fewest pairs in the last step |')
    print('|---|---|---|---|---|---|---|---|')
    for s in (0.02, 0.03, 0.04):
        trials = [(P, G, F.noisy(ds, F.tally_seed(ci, k), s), dm) for ci, P, G, ds, dm in base for k in range(F.TALLY_SEEDS)]
        t = F.tally(trials, intr)
        for side in ('raw', 'filtered'):
            r = t[side]
            print(f"| {s} | {side} | {r['ok']} | {r['trans_le_third']} | {r['rot_le_half']} | {r['worst_rot_ratio']:.2f} | "
                  f"{r['worst_trans_ratio']:.2f} | {r['fewest_pairs']:.0f} |")
        print(f"<!-- s = {s}: more pairs with the filter in {t['more_pairs']} of {t['trials']} trials, smallest ratio {t['smallest_pair_ratio']:.2f} -->")
    clean = [(P, G, ds, dm) for ci, P, G, ds, dm in base]
    for name, points in (('points: true', True), ('points: false', False)):
        t = F.tally(clean, intr, points=points)
        raw, fil = [r['raw'][0] * 1e3 for r in t['records']], [r['filtered'][0] * 1e3 for r in t['records']]
        print(f'clean depth, {name}: raw ends {min(raw):.2f}-{max(raw):.2f} mm from the true pose, filtered {min(fil):.2f}-{max(fil):.2f} mm')
    return 0


if __name__ == '__main__':
    sys.exit(main())
