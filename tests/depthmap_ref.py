"""The Kinect depth map from raw sensor depth, restated in numpy float32: what moped_amd/csrc/depthmap.hip computes,
operation for operation (moped3d/moped3d.cpp:279-333 with cv::resize's bilinear path written out).  The yardstick of
tests/test_gpu_depthmap.py and tests/test_depthmap_cpu.py: every product, difference, quotient, sum and square root is
ONE float32 numpy operation, so the device's correctly rounded single operations give the same bits.

The resize is OpenCV 2.x's generic bilinear path for float as remembered, not as measured: unpinned."""
import numpy as np

F32_M, U16_MM = 0, 1   # MH_RAW_DEPTH_F32_M, MH_RAW_DEPTH_U16_MM
f32 = np.float32
NO_READING = f32(-1e30)


def read_raw(buf, fmt, rw, rh, elem_stride, row_stride, offset):
    """The [rh, rw] float32 map the node's first loop builds (:284-294) from `buf` (bytes-like / uint8 array):
    the value at offset + y row_stride + x elem_stride; NaN / 0 -> -1e30, millimetres times 0.001f."""
    b = np.frombuffer(np.ascontiguousarray(buf).tobytes(), np.uint8)
    es = 4 if fmt == F32_M else 2
    y, x = np.meshgrid(np.arange(rh, dtype=np.int64), np.arange(rw, dtype=np.int64), indexing="ij")
    at = offset + y * row_stride + x * elem_stride
    raw = np.stack([b[at + k] for k in range(es)], -1).copy()
    if fmt == F32_M:
        v = raw.view(np.float32)[..., 0]
        return np.where(np.isnan(v), NO_READING, v).astype(f32)
    mm = raw.view(np.uint16)[..., 0]
    return np.where(mm == 0, NO_READING, mm.astype(f32) * f32(0.001)).astype(f32)


def _coeff(n_dst):
    """Per destination index d: (s, f) with f = (float)((d + 0.5) 0.5 - 0.5), s = floor(f), f -= s."""
    f = ((np.arange(n_dst, dtype=np.float64) + 0.5) * 0.5 - 0.5).astype(f32)
    s = np.floor(f).astype(np.int64)
    return s, (f - s.astype(f32)).astype(f32)


def resize2x(S):
    """S [rh, rw] float32 -> [2 rh, 2 rw]: horizontal pass, then vertical, every product and sum rounded on its own."""
    S = np.ascontiguousarray(S, f32)
    rh, rw = S.shape
    sx, fx = _coeff(2 * rw)
    fx = np.where(sx < 0, f32(0), fx).astype(f32)
    sx = np.maximum(sx, 0)
    last = sx >= rw - 1
    a, b = np.minimum(sx, rw - 1), np.minimum(sx + 1, rw - 1)
    with np.errstate(all="ignore"):
        mix = ((S[:, a] * (f32(1) - fx)).astype(f32) + (S[:, b] * fx).astype(f32)).astype(f32)
        Hm = np.where(last[None, :], S[:, rw - 1:rw], mix).astype(f32)          # [rh, 2 rw]
        sy, fy = _coeff(2 * rh)
        y0, y1 = np.clip(sy, 0, rh - 1), np.clip(sy + 1, 0, rh - 1)
        b0, b1 = (f32(1) - fy).astype(f32), fy
        return ((Hm[y0] * b0[:, None]).astype(f32) + (Hm[y1] * b1[:, None]).astype(f32)).astype(f32)


def data_map(raw, w, h):
    """The depth per pixel of the w x h map before back-projection; beyond the resized map: -1 (any negative is invalid)."""
    rh, rw = raw.shape
    if (w, h) == (rw, rh):
        return raw.astype(f32)
    up = resize2x(raw)
    out = np.full((h, w), f32(-1), f32)
    hh, ww = min(h, 2 * rh), min(w, 2 * rw)
    out[:hh, :ww] = up[:hh, :ww]
    return out


def backproject(data, K):
    """[h, w] depths -> [h, w, 4] (x, y, z, norm); data < 0 -> -1 four times (:317-331)."""
    data = np.ascontiguousarray(data, f32)
    h, w = data.shape
    k = np.asarray(K, f32)
    u = np.arange(w, dtype=f32)[None, :]
    v = np.arange(h, dtype=f32)[:, None]
    with np.errstate(all="ignore"):
        x = ((data * (u - k[2]).astype(f32)).astype(f32) / k[0]).astype(f32)
        y = ((data * (v - k[3]).astype(f32)).astype(f32) / k[1]).astype(f32)
        n = np.sqrt((((x * x).astype(f32) + (y * y).astype(f32)).astype(f32) + (data * data).astype(f32)).astype(f32)).astype(f32)
    out = np.stack([x, y, data, n], -1).astype(f32)
    out[data < 0] = f32(-1)
    return out


def depth_map(buf, fmt, rw, rh, elem_stride, row_stride, offset, K, w, h):
    """The whole of mh_depth_map_from_raw_*: -> [h, w, 4] float32."""
    return backproject(data_map(read_raw(buf, fmt, rw, rh, elem_stride, row_stride, offset), w, h), K)


def plain(z):
    """A plain image of z [rh, rw] (float32 metres or uint16 millimetres) -> the arguments of depth_map up to K."""
    z = np.ascontiguousarray(z)
    fmt = F32_M if z.dtype == np.float32 else U16_MM
    assert fmt == F32_M or z.dtype == np.uint16
    rh, rw = z.shape
    return z.view(np.uint8).reshape(-1), fmt, rw, rh, z.itemsize, rw * z.itemsize, 0


def cloud(z, point_step=16, z_offset=8, row_pad=0, seed=0):
    """An organised PointCloud2-like buffer around z [rh, rw] float32: points of point_step bytes with z at z_offset,
    rows of rw point_step + row_pad bytes, everything else random bytes -> the arguments of depth_map up to K."""
    z = np.ascontiguousarray(z, f32)
    rh, rw = z.shape
    row_step = rw * point_step + row_pad
    buf = np.random.default_rng(seed).integers(0, 256, rh * row_step, dtype=np.uint8)
    zb = z.view(np.uint8).reshape(rh, rw, 4)
    for y in range(rh):
        row = buf[y * row_step:y * row_step + rw * point_step].reshape(rw, point_step)
        row[:, z_offset:z_offset + 4] = zb[y]
    return buf, F32_M, rw, rh, point_step, row_step, z_offset
