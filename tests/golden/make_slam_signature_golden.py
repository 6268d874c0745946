"""
The reference's call signatures of the run -- DF_Prior, Mapper, Tracker, Logger and src/tools/eval_ate.py's functions -- for
tests/test_slam_signatures.py, in the layout of reference_signatures.json.  The reference's modules cannot be imported where this
package is built (they import cv2, colorama, mathutils, ...), so the signatures are read from the parsed source with `ast`;
nothing of the reference is executed.  Build container only.

    python tests/golden/make_slam_signature_golden.py      ->  tests/golden/slam_signatures.json

Per callable: a list of [name, kind, has_default, default] (kind = inspect.Parameter kind name; every default of these
signatures is a literal).
"""
import ast
import json
import os

REF = os.environ.get('ADFP_REFERENCE', '/root/reference')
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'slam_signatures.json')

CLASSES = (('src/DF_Prior.py', 'DF_Prior', ('__init__', 'run')),
           ('src/Mapper.py', 'Mapper', ('__init__', 'run', 'optimize_map', 'keyframe_selection_overlap')),
           ('src/Tracker.py', 'Tracker', ('__init__', 'run', 'optimize_cam_in_batch')),
           ('src/utils/Logger.py', 'Logger', ('__init__', 'log')))
EVAL_ATE = ('src/tools/eval_ate.py', ('associate', 'align', 'plot_traj', 'evaluate_ate', 'evaluate', 'convert_poses'))


def params(fn):
    a = fn.args
    out = []
    positional = list(a.posonlyargs) + list(a.args)
    defaults = [None] * (len(positional) - len(a.defaults)) + list(a.defaults)
    for k, (arg, d) in enumerate(zip(positional, defaults)):
        kind = 'POSITIONAL_ONLY' if k < len(a.posonlyargs) else 'POSITIONAL_OR_KEYWORD'
        out.append([arg.arg, kind, d is not None, ast.literal_eval(d) if d is not None else None])
    if a.vararg is not None:
        out.append([a.vararg.arg, 'VAR_POSITIONAL', False, None])
    for arg, d in zip(a.kwonlyargs, a.kw_defaults):
        out.append([arg.arg, 'KEYWORD_ONLY', d is not None, ast.literal_eval(d) if d is not None else None])
    if a.kwarg is not None:
        out.append([a.kwarg.arg, 'VAR_KEYWORD', False, None])
    json.dumps(out)
    return out


def parsed(rel):
    with open(os.path.join(REF, rel)) as f:
        return ast.parse(f.read())


def main():
    sig = {}
    for rel, cls, names in CLASSES:
        node = next(n for n in parsed(rel).body if isinstance(n, ast.ClassDef) and n.name == cls)
        fns = {n.name: n for n in node.body if isinstance(n, ast.FunctionDef)}
        for name in names:
            sig[f'{cls}.{name}'] = params(fns[name])
    rel, names = EVAL_ATE
    fns = {n.name: n for n in parsed(rel).body if isinstance(n, ast.FunctionDef)}
    for name in names:
        sig[f'eval_ate.{name}'] = params(fns[name])
    lines = ['{"signatures": {']
    for i, (name, ps) in enumerate(sig.items()):
        lines.append(f' {json.dumps(name)}: [\n' + ',\n'.join('  ' + json.dumps(p) for p in ps) + '\n ]' + (',' if i + 1 < len(sig) else ''))
    lines.append('}}')
    with open(OUT, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print(OUT)


if __name__ == '__main__':
    main()
