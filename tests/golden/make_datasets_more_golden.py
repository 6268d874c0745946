"""
The reference's Azure and TUM_RGBD call signatures for tests/test_datasets_tum_host.py, read from the REFERENCE's source text with
`ast` as tests/golden/make_datasets_golden.py reads the other classes'.  Build container only.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_datasets_more_golden.py <reference root>
        ->  tests/golden/datasets_more_signatures.json

Names and argument lists only.  `signatures`: per method, a list of [name, kind, has_default, default].  `attributes`: the names
each class's constructor and loader assign on self.
"""
import ast
import json
import os
import sys

from make_datasets_golden import params, self_names

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'datasets_more_signatures.json')
LOADERS = {'Azure': ['load_poses'], 'TUM_RGBD': []}


def main(ref):
    ds = ast.parse(open(os.path.join(ref, 'src', 'utils', 'datasets.py')).read())
    classes = {n.name: n for n in ds.body if isinstance(n, ast.ClassDef)}
    sig, attrs = {}, {}
    for c in ('Azure', 'TUM_RGBD'):
        methods = [n for n in classes[c].body if isinstance(n, ast.FunctionDef)]
        for m in methods:
            sig[f'{c}.{m.name}'] = params(m)
        attrs[c] = [a for m in methods if m.name == '__init__' or m.name in LOADERS[c] for a in self_names(m)]
    with open(OUT, 'w') as f:
        json.dump({'signatures': sig, 'attributes': attrs}, f, indent=1)
        f.write('\n')
    print(OUT)


if __name__ == '__main__':
    main(sys.argv[1])
