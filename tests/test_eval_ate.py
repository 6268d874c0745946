"""attentive_dfprior_amd.eval_ate on the host: Horn's alignment against scipy's Rotation.align_vectors, the result dict, and
convert_poses' mask.

Bounds: 1e-12 on the RMSE.  Both sides are f64 closed forms of the same optimum (ours Horn's 4 x 4 eigenproblem, scipy's a 3 x 3
SVD) on trajectories of extent ~1 m: the rotation is determined to a few 1e-16 relative by either, and the RMSE of 40 residuals
inherits that times the conditioning of the near-planar case -- an SVD form was seen to differ from scipy by 7e-15 and 2e-15 when
the issue was written.  scipy's `rssd` is the root of the summed squared distances after centring both sets,
so RMSE = rssd / sqrt(n); with a reflection allowed by neither side, both take the proper-rotation optimum."""
import numpy as np
import torch
from scipy.spatial.transform import Rotation

from attentive_dfprior_amd import eval_ate

N = 40
KEYS = ['compared_pose_pairs', 'absolute_translational_error.rmse', 'absolute_translational_error.mean',
        'absolute_translational_error.median', 'absolute_translational_error.std', 'absolute_translational_error.min',
        'absolute_translational_error.max']


def curve(n=N):
    t = np.linspace(0.0, 1.0, n)
    return np.stack([np.cos(3 * t), np.sin(2 * t) + 0.3 * t, 0.5 * t * t + 0.2 * np.sin(5 * t)], 1)       # [n, 3], not planar


def as_dict(xyz):
    return {i: np.concatenate([p, [0, 0, 0, 1]]) for i, p in enumerate(xyz)}


def scipy_rmse(est, gt):
    _, rssd = Rotation.align_vectors(gt - gt.mean(0), est - est.mean(0))
    return rssd / np.sqrt(len(gt))


def test_rigid_motion_is_removed():
    gt = curve()
    R = Rotation.from_rotvec([0.4, -1.1, 0.7]).as_matrix()
    est = gt @ R.T + np.array([0.3, -2.0, 1.5])
    res = eval_ate.evaluate_ate(as_dict(gt), as_dict(est))
    assert list(res.keys()) == KEYS and res['compared_pose_pairs'] == N
    assert res['absolute_translational_error.rmse'] <= 1e-12
    rot, trans, err = eval_ate.align(est.T, gt.T)
    assert isinstance(rot, np.ndarray) and not isinstance(rot, np.matrix) and rot.shape == (3, 3) and trans.shape == (3, 1) and err.shape == (N,)
    assert np.abs(rot - R.T).max() <= 1e-12 and abs(np.linalg.det(rot) - 1) <= 1e-12


def test_noise_agrees_with_scipy():
    gt = curve()
    R = Rotation.from_rotvec([0.4, -1.1, 0.7]).as_matrix()
    est = gt @ R.T + np.array([0.3, -2.0, 1.5]) + np.random.default_rng(7).normal(0, 0.01, gt.shape)
    res = eval_ate.evaluate_ate(as_dict(gt), as_dict(est))
    want = scipy_rmse(est, gt)
    print('noise: rmse', res['absolute_translational_error.rmse'], 'scipy', want, 'difference', abs(res['absolute_translational_error.rmse'] - want))
    assert 0.005 < want < 0.03 and abs(res['absolute_translational_error.rmse'] - want) <= 1e-12
    err = eval_ate.align(est.T, gt.T)[2]
    assert res['absolute_translational_error.mean'] == np.mean(err) and res['absolute_translational_error.median'] == np.median(err)
    assert res['absolute_translational_error.std'] == np.std(err) and res['absolute_translational_error.min'] == np.min(err)
    assert res['absolute_translational_error.max'] == np.max(err)


def test_mirrored_near_planar_trajectory_takes_the_reflection_branch():
    rng = np.random.default_rng(11)
    t = np.linspace(0, 1, N)
    gt = np.stack([np.cos(4 * t), np.sin(3 * t), 1e-3 * rng.normal(size=N)], 1)
    est = gt * np.array([1.0, 1.0, -1.0]) + rng.normal(0, 1e-4, gt.shape)            # mirrored through the trajectory's plane
    a, b = est - est.mean(0), gt - gt.mean(0)
    U, _, Vh = np.linalg.svd((a.T @ b).T)
    assert np.linalg.det(U) * np.linalg.det(Vh) < 0                                  # the unconstrained optimum IS a reflection
    rot, _, _ = eval_ate.align(est.T, gt.T)
    assert abs(np.linalg.det(rot) - 1) <= 1e-12                                      # ... and align returns a rotation
    res = eval_ate.evaluate_ate(as_dict(gt), as_dict(est))
    want = scipy_rmse(est, gt)
    print('mirror: rmse', res['absolute_translational_error.rmse'], 'scipy', want, 'difference', abs(res['absolute_translational_error.rmse'] - want))
    assert abs(res['absolute_translational_error.rmse'] - want) <= 1e-12 and want > 1e-4


def test_identical_trajectories_give_exactly_zero():
    """For identical trajectories the cross-covariance is exactly symmetric, Horn's 4 x 4 matrix decouples exactly and the
    rotation is the identity bit for bit: every error is +0.0, whatever the trajectory (float32 poses as a run stores them,
    3 to 60 points, extents from centimetres to tens of metres, far from the origin, planar and collinear ones too)."""
    rng = np.random.default_rng(5)
    shapes = [rng.normal(size=(int(rng.integers(3, 60)), 3)) * rng.uniform(0.01, 30) + rng.normal(size=3) * 20 for _ in range(200)]
    shapes += [curve(), curve() * np.array([1.0, 1.0, 0.0]), np.outer(np.linspace(0, 1, 9), [0.3, -0.2, 0.9])]
    for xyz in shapes:
        xyz = xyz.astype(np.float32).astype(np.float64)
        rot, trans, err = eval_ate.align(xyz.T, xyz.T.copy())
        assert np.array_equal(rot, np.eye(3)) and not trans.any() and not err.any(), (xyz.shape, rot, trans, err.max())
        res = eval_ate.evaluate_ate(as_dict(xyz), as_dict(xyz.copy()))
        assert all(res[k] == 0.0 for k in KEYS[1:]) and res['compared_pose_pairs'] == len(xyz)


def test_associate_and_too_few_matches():
    assert eval_ate.associate({0.0: 1, 1.0: 2, 2.0: 3}, {0.01: 1, 1.015: 2, 5.0: 3}) == [(0.0, 0.01), (1.0, 1.015)]
    assert eval_ate.associate({0.0: 1}, {0.05: 1}, offset=-0.04) == [(0.0, 0.05)]
    try:
        eval_ate.evaluate_ate({0: [0, 0, 0]}, {0: [0, 0, 0]})
    except ValueError:
        pass
    else:
        raise AssertionError('one pair must be refused')


def test_convert_poses_masks_non_finite_ground_truth_and_copies():
    c2w = torch.eye(4).repeat(5, 1, 1)
    c2w[:, :3, 3] = torch.arange(15, dtype=torch.float32).reshape(5, 3)
    c2w[1, 0, 0] = float('inf')
    c2w[3, 2, 3] = float('nan')
    before = c2w.clone()
    poses, mask = eval_ate.convert_poses(c2w, 4, 2.0)
    assert mask.tolist() == [True, False, True, False, True] and tuple(poses.shape) == (3, 7)
    assert torch.equal(poses[:, :3], before[[0, 2, 4], :3, 3] / 2.0)                 # translation first, divided by scale
    assert torch.equal(poses[:, 3:], torch.tensor([[1.0, 0, 0, 0]] * 3))
    assert before.view(torch.int32).equal(c2w.view(torch.int32))                     # the input is untouched, bit for bit
    est, m2 = eval_ate.convert_poses(torch.eye(4).repeat(5, 1, 1), 4, 2.0, gt=False)                          # the estimate's list is never masked
    assert m2.all() and tuple(est.shape) == (5, 7)


def test_evaluate_and_ate_of_lists(capsys):
    gt = torch.eye(4).repeat(6, 1, 1)
    gt[:, :3, 3] = torch.from_numpy(curve(6)).float()
    est = gt.clone()
    est[:, 0, 3] += 0.25
    gt[2] = float('nan')
    res = eval_ate.ate_of_lists(gt, est, 5, 1.0)
    assert res['compared_pose_pairs'] == 5 and res['absolute_translational_error.rmse'] <= 1e-6
    pg, mask = eval_ate.convert_poses(gt, 5, 1.0)
    pe, _ = eval_ate.convert_poses(est, 5, 1.0)
    out = eval_ate.evaluate(pg, pe[mask], plot='')
    assert out['compared_pose_pairs'] == 5 and 'absolute_translational_error.rmse' in capsys.readouterr().out
    assert eval_ate.ate_of_lists(gt[:1], est[:1], 0, 1.0) is None
