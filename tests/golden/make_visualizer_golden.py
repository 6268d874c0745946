"""
The reference's Visualizer call signatures for tests/test_vis_host.py, read from the REFERENCE's source text with `ast`
(src/utils/Visualizer.py imports open3d and matplotlib, so it cannot be imported where they are missing).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_visualizer_golden.py <reference root>   ->  tests/golden/visualizer_signatures.json

Names and argument lists only.  Per callable: a list of [name, kind, has_default, default] as in datasets_signatures.json.
`attributes`: the names Visualizer.__init__ assigns on self.
"""
import ast
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_datasets_golden import params, self_names          # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'visualizer_signatures.json')


def main(ref):
    tree = ast.parse(open(os.path.join(ref, 'src', 'utils', 'Visualizer.py')).read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == 'Visualizer')
    method = lambda m: next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == m)
    sig = {f'Visualizer.{m}': params(method(m)) for m in ('__init__', 'vis')}
    with open(OUT, 'w') as f:
        json.dump({'signatures': sig, 'attributes': self_names(method('__init__'))}, f, indent=1)
        f.write('\n')
    print(OUT)


if __name__ == '__main__':
    main(sys.argv[1])
