"""
The reference's public call signatures and the DF module's state-dict layout, read from the REFERENCE's own classes and functions
(imported read-only through oracle/ref_import.py), for tests/test_api_signatures.py.  Build container only.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_signature_golden.py      ->  tests/golden/reference_signatures.json

Per callable: a list of [name, kind, has_default, default] (kind = inspect.Parameter kind name; every default of these
signatures is None, a number, a string, a bool or a list).  `state_dict`: [key, shape] in the module's order.
"""
import inspect
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import ref_import                # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'reference_signatures.json')

RENDERER = ('__init__', 'eval_points', 'sample_grid_tsdf', 'eval_points_tsdf', 'render_batch_ray', 'render_img')
COMMON = ('get_rays', 'get_rays_from_uv', 'select_uv', 'get_sample_uv', 'get_samples', 'raw2outputs_nerf_color',
          'normalize_3d_coordinate', 'random_select')


def params(fn):
    out = []
    for p in inspect.signature(fn).parameters.values():
        has = p.default is not inspect.Parameter.empty
        d = p.default if has else None
        if isinstance(d, tuple):
            d = list(d)
        json.dumps(d)                            # fails loudly on a default JSON cannot hold
        out.append([p.name, p.kind.name, has, d])
    return out


def main():
    rcommon, rdecoder, rrenderer = ref_import.load()
    sig = {f'Renderer.{n}': params(getattr(rrenderer.Renderer, n)) for n in RENDERER}
    sig['DF.__init__'] = params(rdecoder.DF.__init__)
    sig['DF.forward'] = params(rdecoder.DF.forward)
    sig['MLP.__init__'] = params(rdecoder.MLP.__init__)
    sig.update({f'common.{n}': params(getattr(rcommon, n)) for n in COMMON})
    sd = rdecoder.DF(dim=3, c_dim=32, low_grid_len=0.32, high_grid_len=0.16, color_grid_len=0.16, hidden_size=32,
                     pos_embedding_method='fourier').state_dict()
    lines = ['{"signatures": {']
    for i, (name, ps) in enumerate(sig.items()):
        lines.append(f' {json.dumps(name)}: [\n' + ',\n'.join('  ' + json.dumps(p) for p in ps) + '\n ]' + (',' if i + 1 < len(sig) else ''))
    lines.append('}, "state_dict": [')
    lines.append(',\n'.join(' ' + json.dumps([k, list(v.shape)]) for k, v in sd.items()))
    lines.append(']}')
    with open(OUT, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print(OUT)


if __name__ == '__main__':
    main()
