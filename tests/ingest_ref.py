"""Host statement of frame ingestion (the chain of the reference's BaseDataset.__getitem__, src/utils/datasets.py:77-113, from the
decoded bytes on; include/adfp.h "frame ingestion").  A helper, not a test.

Steps A (bytes / 255 in f64), B (cv2.resize on doubles, restated: float coefficients, f64 products, horizontal pass first) and D
(the edge crop) are numpy; step C (cfg cam.crop_size) calls torch.nn.functional.interpolate itself on CPU tensors -- float64
colour in the reference's permuted layout, float32 depth -- so that stage is the reference's own library, not a restatement."""
import numpy as np
import torch
import torch.nn.functional as F


def out_shape(depth_hw, crop_size=None, crop_edge=0):
    h, w = crop_size if crop_size else depth_hw
    return h - 2 * crop_edge, w - 2 * crop_edge


def cv_coef(dst_n, src_n):
    """OpenCV's linear coefficients: the source position in f64 rounded to float, its floor and the float remainder."""
    d = np.arange(dst_n, dtype=np.float64)
    f = ((d + 0.5) * np.float64(src_n) / np.float64(dst_n) - 0.5).astype(np.float32)
    fl = np.floor(f)
    return fl.astype(np.int64), (f - fl).astype(np.float32)


def cv_resize_f64(img, dst_hw):
    """cv2.resize(img, (W, H)) for a float64 [h, w, c] image, INTER_LINEAR."""
    h, w = img.shape[:2]
    H, W = dst_hw
    sx, fx = cv_coef(W, w)
    lo, hi = sx < 0, sx >= w - 1
    sx = np.where(lo, 0, np.where(hi, w - 1, sx))
    fx = np.where(lo | hi, np.float32(0), fx).astype(np.float32)
    sx1 = np.minimum(sx + 1, w - 1)
    a0 = (np.float32(1) - fx).astype(np.float64)[None, :, None]
    a1 = fx.astype(np.float64)[None, :, None]
    hor = img[:, sx] * a0 + img[:, sx1] * a1                    # [h, W, c]
    sy, fy = cv_coef(H, h)
    y0, y1 = np.clip(sy, 0, h - 1), np.clip(sy + 1, 0, h - 1)   # rows clamped, weights kept
    b0 = (np.float32(1) - fy).astype(np.float64)[:, None, None]
    b1 = fy.astype(np.float64)[:, None, None]
    return hor[y0] * b0 + hor[y1] * b1


def ingest(color_u8, depth_raw, png_depth_scale, scale=1.0, crop_size=None, crop_edge=0, color_order='rgb'):
    """(colour [H,W,3] float64, depth [H,W] float32) as numpy arrays."""
    color_u8 = np.asarray(color_u8)
    rgb = color_u8[..., ::-1] if color_order == 'bgr' else color_u8
    color = rgb / 255.
    depth = np.asarray(depth_raw).astype(np.float32) / png_depth_scale
    H, W = depth.shape
    if color.shape[:2] != (H, W):
        color = cv_resize_f64(color, (H, W))
    color = torch.from_numpy(np.ascontiguousarray(color))
    depth = torch.from_numpy(depth) * scale
    if crop_size:
        color = color.permute(2, 0, 1)
        color = F.interpolate(color[None], list(crop_size), mode='bilinear', align_corners=True)[0]
        depth = F.interpolate(depth[None, None], list(crop_size), mode='nearest')[0, 0]
        color = color.permute(1, 2, 0).contiguous()
    if crop_edge > 0:
        color = color[crop_edge:-crop_edge, crop_edge:-crop_edge]
        depth = depth[crop_edge:-crop_edge, crop_edge:-crop_edge]
    assert color.dtype == torch.float64 and depth.dtype == torch.float32
    return color.contiguous().numpy(), depth.contiguous().numpy()
