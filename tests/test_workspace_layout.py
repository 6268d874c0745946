"""CPU: every workspace / index size query of the mesh tools and of the render path (adfp_workspace_bytes,
adfp_backward_workspace_bytes) returns what tests/golden/workspace_bytes.json recorded.  The launchers
carve their workspaces with the same layout functions that answer these queries (csrc/adfp_host.h's Arena), so a fixed table of
sizes pins the layouts: a buffer added, dropped, reordered or rounded differently moves a number here.  The table was recorded from
the build before the layouts moved to the arena; `python tests/test_workspace_layout.py` rewrites it from the current build, which
is only right after a deliberate, ABI-versioned layout change.

The argument grid: 0, negative, 1, 255 / 256 / 257 (the alignment), one below, at and above the tile sizes 1024, 2048, 4096, 10^6,
and every tool's "too large" limit and limit + 1 (RECON_MAX_N = 2^31 - 1 - 1024, a third of it for meshes, 2^40 ids for the bound)."""
import json
import os

from attentive_dfprior_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'workspace_bytes.json')

RECON_MAX_N = 0x7fffffff - 1024
BND_MAX_IDS = 1 << 40
SIZES = [-1, 0, 1, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 10 ** 6,
         RECON_MAX_N // 3, RECON_MAX_N // 3 + 1, RECON_MAX_N, RECON_MAX_N + 1, BND_MAX_IDS, BND_MAX_IDS + 1]
FEW = [-1, 0, 1, 256, 257, 2048, 2049, 4097, 10 ** 6, RECON_MAX_N // 3, RECON_MAX_N // 3 + 1, RECON_MAX_N, RECON_MAX_N + 1]

ONE_ARG = ['adfp_sort_workspace_bytes', 'adfp_nn_index_bytes', 'adfp_nn_build_workspace_bytes', 'adfp_recon_reduce_workspace_bytes',
           'adfp_sample_surface_workspace_bytes', 'adfp_tri_bvh_build_workspace_bytes', 'adfp_vertex_normals_workspace_bytes',
           'adfp_voxel_down_sample_workspace_bytes', 'adfp_mesh_face_labels_workspace_bytes',
           'adfp_mesh_component_keep_workspace_bytes', 'adfp_mesh_merge_workspace_bytes', 'adfp_bound_classify_workspace_bytes',
           'adfp_workspace_bytes', 'adfp_backward_workspace_bytes']
MC_SHAPES = [(0, 4, 4), (4, -1, 4), (4, 4, 0), (1, 1, 1), (2, 2, 2), (1, 1, 1023), (1, 1024, 1), (1025, 1, 1), (16, 16, 8), (8, 16, 16),
             (3, 5, 7), (17, 31, 65), (100, 100, 100), (257, 129, 33), (512, 512, 512), (2048, 2048, 2048), (1290, 1290, 1290)]
BOUND_SHAPES = [(0, 4, 4, 8), (-1, 4, 4, 8), (1, 0, 4, 8), (1, 4, 0, 8), (1, 4, 4, 0), (1, 1, 1, 1), (1, 4, 4, 8), (3, 17, 31, 26),
                (1, 31, 33, 1024), (1, 31, 33, 1025), (2, 480, 640, 162), (40, 680, 1200, 642), (1, 32768, 32768, 6),
                (1, 32769, 8, 6), (1, 8, 32769, 6), (1024, 32768, 32768, 6), (1025, 32768, 32768, 6), (BND_MAX_IDS // 2, 1, 1, 6),
                (BND_MAX_IDS // 2 + 1, 1, 1, 6)]


def queries():
    """(name, args) of every pinned query, in a fixed order."""
    q = [(name, (n,)) for name in ONE_ARG for n in SIZES]
    q += [('adfp_nn_query_workspace_bytes', (n, flags)) for flags in (0, 1) for n in FEW]
    q += [('adfp_tri_bvh_bytes', (n, leaf)) for leaf in (4, 8, 16, 5, 0) for n in FEW + [3, 4, 5, 15, 16, 17, 64, 65]]
    q += [('adfp_depth_l1_workspace_bytes', (v, p)) for v in (-1, 0, 1, 7, 32768, 32769, RECON_MAX_N, RECON_MAX_N + 1)
          for p in (-1, 0, 1, 255, 256, 257, 640 * 480, 262143, 262144, 262145, RECON_MAX_N, RECON_MAX_N + 1)]
    q += [('adfp_mesh_compact_workspace_bytes', (v, f)) for v in FEW for f in FEW]
    q += [('adfp_mc_workspace_bytes', s) for s in MC_SHAPES]
    q += [('adfp_bound_support_workspace_bytes', s) for s in BOUND_SHAPES]
    return q


def measure():
    L = _lib.lib()
    return [[name, list(args), int(getattr(L, name)(*args))] for name, args in queries()]


def test_workspace_sizes_match_the_recorded_table():
    golden = json.load(open(GOLDEN))
    assert [(n, tuple(a)) for n, a, _ in golden] == queries(), 'the golden table and the argument grid differ'
    L = _lib.lib()
    wrong = [(n, a, want, int(getattr(L, n)(*a))) for n, a, want in golden if int(getattr(L, n)(*a)) != want]
    assert not wrong, f'{len(wrong)} size queries moved, the first: {wrong[:5]}'
    assert sum(1 for _, _, v in golden if v) > len(golden) // 3              # the table is not a table of refusals


if __name__ == '__main__':
    with open(GOLDEN, 'w') as f:
        f.write('[\n' + ',\n'.join(json.dumps(row) for row in measure()) + '\n]\n')
