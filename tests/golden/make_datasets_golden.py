"""
The reference's dataset and prior-volume call signatures for tests/test_ingest_host.py, read from the REFERENCE's source text with
`ast` (src/utils/datasets.py imports cv2 and get_tsdf.py imports open3d, so neither can be imported here).  Build container only.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_datasets_golden.py [reference root]   ->  tests/golden/datasets_signatures.json

Names and argument lists only.  Per callable: a list of [name, kind, has_default, default] as in reference_signatures.json.
`dataset_dict`: config name -> class name.  `attributes`: the names BaseDataset.__init__ and the two loaders' constructors assign
on self.
"""
import ast
import json
import os
import sys

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'datasets_signatures.json')


def params(fn):
    a = fn.args
    assert not a.posonlyargs and not a.kwonlyargs and a.vararg is None and a.kwarg is None, fn.name
    first = len(a.args) - len(a.defaults)
    out = []
    for i, arg in enumerate(a.args):
        has = i >= first
        out.append([arg.arg, 'POSITIONAL_OR_KEYWORD', has, ast.literal_eval(a.defaults[i - first]) if has else None])
    return out


def self_names(fn):
    names = []
    for node in ast.walk(fn):
        targets = node.targets if isinstance(node, ast.Assign) else []
        for t in targets:
            for e in (t.elts if isinstance(t, ast.Tuple) else [t]):
                if isinstance(e, ast.Attribute) and isinstance(e.value, ast.Name) and e.value.id == 'self' and e.attr not in names:
                    names.append(e.attr)
    return names


def main(ref):
    ds = ast.parse(open(os.path.join(ref, 'src', 'utils', 'datasets.py')).read())
    gt = ast.parse(open(os.path.join(ref, 'get_tsdf.py')).read())
    fns = {n.name: n for n in ds.body if isinstance(n, ast.FunctionDef)}
    classes = {n.name: n for n in ds.body if isinstance(n, ast.ClassDef)}
    method = lambda c, m: next(n for n in classes[c].body if isinstance(n, ast.FunctionDef) and n.name == m)
    gfn = {n.name: n for n in gt.body if isinstance(n, ast.FunctionDef)}
    sig = {'get_dataset': params(fns['get_dataset'])}
    for c in ('BaseDataset', 'Replica', 'ScanNet'):
        sig[f'{c}.__init__'] = params(method(c, '__init__'))
    sig['BaseDataset.__getitem__'] = params(method('BaseDataset', '__getitem__'))
    sig['update_cam'] = params(gfn['update_cam'])
    sig['init_tsdf_volume'] = params(gfn['init_tsdf_volume'])
    table = next(n for n in ds.body if isinstance(n, ast.Assign) and n.targets[0].id == 'dataset_dict').value
    dataset_dict = {k.value: v.id for k, v in zip(table.keys, table.values)}
    attrs = {c: self_names(method(c, '__init__')) + (self_names(method(c, 'load_poses')) if c != 'BaseDataset' else [])
             for c in ('BaseDataset', 'Replica', 'ScanNet')}
    with open(OUT, 'w') as f:
        json.dump({'signatures': sig, 'dataset_dict': dataset_dict, 'attributes': attrs}, f, indent=1)
        f.write('\n')
    print(OUT)


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else '/root/reference')
