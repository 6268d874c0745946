"""Host statement of lens undistortion (include/adfp.h "lens undistortion"): the 1/32-pixel fixed-point map in float64 and the
bilinear remap in int64, both numpy.  A helper, not a test.

The rule is this package's own: it follows the scheme of cv2.undistort(img, K, dist) with newCameraMatrix = K (fixed-point map,
bilinear taps, constant border 0) and has not been compared with cv2, which is not a dependency."""
import numpy as np

SENTINEL = np.iinfo(np.int32).min
LIMIT = float(2 ** 30)

# (h, w), fx, fy, cx, cy, dist: two tiny geometries, the 8-coefficient model, a denominator that crosses zero inside the image
# (non-finite and far-away entries), and TUM freiburg1's and freiburg2's calibrations
GEOMETRIES = [
    ((6, 8), 30.0, 31.0, 3.5, 2.5, [0.4, 0.1, 0.02, -0.03]),
    ((37, 53), 40.0, 41.0, 25.5, 17.5, [0.35, -0.2, 0.01, -0.008, 0.05]),
    ((37, 53), 40.0, 41.0, 25.5, 17.5, [0.35, -0.2, 0.01, -0.008, 0.05, 0.1, -0.05, 0.02]),
    ((37, 53), 40.0, 41.0, 25.5, 17.5, [0.0, 0, 0, 0, 0, -4.0, 0, 0]),
    ((480, 640), 517.3, 516.5, 318.6, 255.3, [0.2624, -0.9531, -0.0054, 0.0026, 1.1633]),
    ((480, 640), 520.9, 521.0, 325.1, 249.7, [0.2312, -0.7849, -0.0033, -0.0001, 0.9172]),
]
FREIBURG1 = GEOMETRIES[4]


def undistort_map(hw, fx, fy, cx, cy, dist):
    """[h, w, 2] int32: (iu, iv) per pixel."""
    h, w = hw
    k = np.zeros(8, dtype=np.float64)
    k[:len(dist)] = dist
    k1, k2, p1, p2, k3, k4, k5, k6 = k
    fx, fy, cx, cy = (np.float64(v) for v in (fx, fy, cx, cy))
    v, u = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing='ij')
    with np.errstate(all='ignore'):
        x = (u - cx) / fx
        y = (v - cy) / fy
        r2 = x * x + y * y
        kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
        xd = x * kr + p1 * (2 * x * y) + p2 * (r2 + 2 * (x * x))
        yd = y * kr + p1 * (r2 + 2 * (y * y)) + p2 * (2 * x * y)
        U = fx * xd + cx
        V = fy * yd + cy
        finite = np.isfinite(U) & np.isfinite(V)
        iu = np.rint(np.clip(32 * np.where(finite, U, 0.0), -LIMIT, LIMIT)).astype(np.int64)
        iv = np.rint(np.clip(32 * np.where(finite, V, 0.0), -LIMIT, LIMIT)).astype(np.int64)
    out = np.stack([np.where(finite, iu, SENTINEL), np.where(finite, iv, SENTINEL)], axis=-1)
    return out.astype(np.int32)


def identity_map(hw):
    h, w = hw
    v, u = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    return (32 * np.stack([u, v], axis=-1)).astype(np.int32)


def remap(img, m):
    """uint8 [h, w, c] through the map [h, w, 2]: four taps, 0 outside the image, weights in 1/1024ths."""
    img = np.asarray(img)
    h, w = img.shape[:2]
    m = np.asarray(m).astype(np.int64)
    iu, iv = m[..., 0], m[..., 1]
    sx, sy, a, b = iu >> 5, iv >> 5, iu & 31, iv & 31
    src = img.astype(np.int64)

    def tap(yy, xx):
        inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        return np.where(inside[..., None], src[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)], 0)

    a, b = a[..., None], b[..., None]
    acc = (32 - a) * (32 - b) * tap(sy, sx) + a * (32 - b) * tap(sy, sx + 1) + (32 - a) * b * tap(sy + 1, sx) + a * b * tap(sy + 1, sx + 1)
    out = (acc + 512) >> 10
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)
