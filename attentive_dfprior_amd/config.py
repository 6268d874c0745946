"""Drop-in for the reference's ``src/config.py``: ``load_config(path, default_path=None)`` with its ``inherit_from`` chain and
recursive update, ``update_recursive`` and ``get_model(cfg)``.  yaml alone is needed: the reference's module imports ``conv_onet``.

The run and every tool of this package take the default config as ``configs/df_prior.yaml`` relative to the working directory
(``--default_config`` replaces it), as the reference's ``run.py`` does."""
import yaml

from . import get_model  # noqa: F401  (src/config.py:63-78 forwards to the same factory)

DEFAULT_CONFIG = 'configs/df_prior.yaml'

# Settings the reference's config files do not carry (it dropped its parent project's bundle adjustment); a config that names
# them wins.  ``load_config`` returns the files' content unchanged: readers ask ``mapping_setting``.
MAPPING_DEFAULTS = {'BA': False, 'BA_cam_lr': 0.0002}


def mapping_setting(cfg, key):
    """``cfg['mapping'][key]``, or this package's default for a key the reference's configs do not have."""
    m = cfg.get('mapping') or {}
    return m[key] if key in m else MAPPING_DEFAULTS[key]


# tracking.init: what a tracked frame starts from.  'guess' = the constant-speed guess as it is (the reference's path, and what an
# absent key means); 'icp' = the guess refined by icp.DepthICP, point-to-plane ICP of the whole depth image against the raycast of
# the TSDF prior -- with tracking.iters: 0 that result is the frame's pose.  tracking.icp: keywords of DepthICP's constructor
# (strides, iters, dist_tol, cos_tol, min_pivot, min_pairs, max_jump, max_shift, max_angle, near, bilateral); lengths are metres and
# are NOT multiplied by `scale`.  tracking.icp.bilateral: {radius, sigma_space, sigma_depth, sigma_depth_z2, points} -- the ICP reads
# the sensor depth through icp.depth_bilateral ({}: its defaults; absent, None or False: off).  tracking.icp_rgb: {'weight': w, 'tol': t} -- with tracking.init: icp and w > 0 (absent or 0: off) every ICP
# step adds a photometric term against the last tracked frame, weighted by w, to its normal equations (icp.RgbdICP; t drops pairs
# whose intensities differ by more, RgbdICP's default when absent).  A weight > 0 without tracking.init: icp is an error.
TRACKING_DEFAULTS = {'init': 'guess', 'icp': {}, 'icp_rgb': {}}
TRACKING_INITS = ('guess', 'icp')


def tracking_setting(cfg, key):
    """``cfg['tracking'][key]``, or this package's default for a key the reference's configs do not have."""
    t = cfg.get('tracking') or {}
    return t[key] if key in t else TRACKING_DEFAULTS[key]


# meshing.simplify_voxel_size: None or 0 = the marching-cubes mesh as it is; a positive number = the voxel (in the config's units,
# multiplied by `scale` like the bounds) of mesh.simplify_vertex_clustering, run by Mesher.mesh_arrays after the component clean-up
# and before the colour query.  meshing.simplify_contraction: 'quadric' or 'average'.  (Vertex clustering by this package's own
# rules, include/adfp.h "mesh simplification": open3d's simplify_vertex_clustering was never run against it.)
MESHING_DEFAULTS = {'simplify_voxel_size': None, 'simplify_contraction': 'quadric'}


# color_mesh_extraction_method: keyframe_projection (mesher.Mesher, mesh.project_colors): projection_depth_tol = how far, in the
# config's units (multiplied by `scale`), a keyframe's depth may lie from the vertex's for the keyframe to count as seeing it --
# 0.05 is the 5 cm the completion ratio and the F-score call "the same surface"; projection_blend 'weighted' (cos / depth^2 over all
# views) or 'best' (the view of largest weight alone); projection_border = pixels kept clear of the image's edge.
PROJECTION_DEFAULTS = {'projection_depth_tol': 0.05, 'projection_blend': 'weighted', 'projection_border': 0}


def meshing_setting(cfg, key):
    """``cfg['meshing'][key]``, or this package's default for a key the reference's configs do not have."""
    m = cfg.get('meshing') or {}
    if key in m:
        return m[key]
    return MESHING_DEFAULTS[key] if key in MESHING_DEFAULTS else PROJECTION_DEFAULTS[key]


def load_config(path, default_path=None):
    """The config of `path` merged over what it inherits: its ``inherit_from`` file (recursively), else `default_path`, else
    nothing (src/config.py:10-42)."""
    with open(path, 'r') as f:
        cfg_special = yaml.full_load(f)
    inherit_from = cfg_special.get('inherit_from')
    if inherit_from is not None:
        cfg = load_config(inherit_from, default_path)
    elif default_path is not None:
        with open(default_path, 'r') as f:
            cfg = yaml.full_load(f)
    else:
        cfg = dict()
    update_recursive(cfg, cfg_special)
    return cfg


def update_recursive(dict1, dict2):
    """`dict2`'s entries written into `dict1`, dictionaries merged key by key (src/config.py:45-59)."""
    for k, v in dict2.items():
        if k not in dict1:
            dict1[k] = dict()
        if isinstance(v, dict):
            update_recursive(dict1[k], v)
        else:
            dict1[k] = v
