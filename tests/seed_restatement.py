"""float64 restatement of scene seeding (the numerical part of the reference's scene_initialization, train.py:58-199)
in numpy, written step by step from the formulas and sharing no code with mobgs_amd or the kernel: it is what the
GPU tests compare against, and tests/golden/make_golden_seed.py stores its results next to the reference's own fp32
ones.  Only the track search is evaluated in float32 on purpose: the argmin is defined on fp32 distances."""
import numpy as np

BORDER = 1e-3   # px: a reprojection this close to the image border may fall on either side in fp32


def world_points(depths, w2c, K):
    """[V,H,W,3]: R^T (d K^-1 [u, v, 1]) - R^T t."""
    d = np.asarray(depths, np.float64)
    V, H, W = d.shape
    vv, uu = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    pix = np.stack([uu, vv, np.ones_like(uu)], -1)                      # [H,W,3]
    out = np.empty((V, H, W, 3))
    for i in range(V):
        R, t = np.asarray(w2c[i], np.float64)[:, :3], np.asarray(w2c[i], np.float64)[:, 3]
        cam = (pix @ np.linalg.inv(np.asarray(K[i], np.float64)).T) * d[i][..., None]
        out[i] = cam @ R - R.T @ t                                      # rows: (R^T cam)^T = cam^T R
    return out


def consistency(images, depths, w2c, K):
    """-> (accum_error [V,H,W], mean [V], near_border [V,H,W] bool).  near_border: some reprojection of the pixel into
    ANOTHER view lies within BORDER px of that view's in/out boundary (x = 0, x = W - 1, y = 0, y = H - 1)."""
    img = np.asarray(images, np.float64)
    V, _, H, W = img.shape
    world = world_points(depths, w2c, K).reshape(V, -1, 3)
    accum = np.zeros((V, H * W))
    near = np.zeros((V, H * W), bool)
    for i in range(V):
        tgt = img[i].reshape(3, -1)
        for j in range(V):
            R, t, k = np.asarray(w2c[j], np.float64)[:, :3], np.asarray(w2c[j], np.float64)[:, 3], np.asarray(K[j], np.float64)
            cam = world[i] @ R.T + t
            z = np.where(np.abs(cam[:, 2]) < 1e-6, 1e-6, cam[:, 2])
            p = (cam / z[:, None]) @ k.T
            x, y = p[:, 0], p[:, 1]
            if j != i:
                near[i] |= (np.minimum(np.abs(x), np.abs(x - (W - 1))) < BORDER) | \
                           (np.minimum(np.abs(y), np.abs(y - (H - 1))) < BORDER)
            xn, yn = 2 * x / (W - 1) - 1, 2 * y / (H - 1) - 1
            inside = (xn >= -1) & (xn <= 1) & (yn >= -1) & (yn <= 1)
            ix, iy = (xn + 1) / 2 * (W - 1), (yn + 1) / 2 * (H - 1)
            x0, y0 = np.floor(ix), np.floor(iy)
            s = np.zeros((3, H * W))
            src = img[j].reshape(3, -1)
            for ox in (0, 1):
                for oy in (0, 1):
                    xs, ys = x0 + ox, y0 + oy
                    ok = inside & (xs >= 0) & (xs <= W - 1) & (ys >= 0) & (ys <= H - 1)
                    wgt = np.where(ok, (1 - np.abs(ix - xs)) * (1 - np.abs(iy - ys)), 0.0)
                    at = np.where(ok, ys * W + xs, 0).astype(np.int64)
                    s += wgt * src[:, at]
            mask = s.sum(0) > 0
            accum[i] += np.where(mask, np.abs(s - tgt).sum(0) / 3.0, 0.0)
    return accum.reshape(V, H, W), accum.mean(1), near.reshape(V, H, W)


def classify(accum, mean, motion):
    """-> (inconsistent uint8, cls uint8): 0 static candidate, 1 dynamic candidate, 2 neither."""
    inc = np.asarray(accum) > np.asarray(mean)[:, None, None]
    mo = np.asarray(motion)
    cls = np.full(inc.shape, 2, np.uint8)
    cls[~inc & (mo == 0)] = 0
    cls[inc & (mo == 1)] = 1
    return inc.astype(np.uint8), cls


def nearest_pixel(u):
    """nearbyint(u - 0.5), ties to even (np.rint)."""
    return np.rint(np.asarray(u, np.float64) - 0.5)


def track_lookup(coords, tracklet, H, W):
    """-> (track_index [N] int64, pixel [N,T] int64: y * W + x of the sampled pixel, -1 where the track is outside).
    Distances are float32 (dx dx + dy dy), first minimum wins."""
    c = np.asarray(coords, np.float32)
    tr = np.asarray(tracklet, np.float32)
    dx = c[:, None, 0] - tr[0][None, :, 0]
    dy = c[:, None, 1] - tr[0][None, :, 1]
    dist = dx * dx + dy * dy
    assert dist.dtype == np.float32
    index = dist.argmin(1)
    uv = tr[:, index, :]                                                # [T,N,2]
    x, y = nearest_pixel(uv[..., 0]), nearest_pixel(uv[..., 1])
    ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
    pixel = np.where(ok, y * W + x, -1).astype(np.int64)
    return index.astype(np.int64), pixel.T


def gather_trajectory(points, pixel):
    """points [V,H,W,3], pixel [N,T] -> [N,T,3] in the dtype of `points`: a pure gather, zeros where pixel < 0."""
    pts = np.asarray(points)
    V = pts.shape[0]
    flat = pts.reshape(V, -1, 3)
    out = np.zeros(pixel.shape + (3,), pts.dtype)
    for t in range(V):
        ok = pixel[:, t] >= 0
        out[ok, t] = flat[t][pixel[ok, t]]
    return out


def clouds(images, points, cls, times, stat_idx, dyn_idx):
    """The point clouds for given picks: stat_idx indexes the static candidates of all views (view-major), dyn_idx the
    dynamic candidates of view 0.  -> dict(stat_points, stat_colors, stat_times, dyn_points, dyn_colors, dyn_times,
    dyn_coords)."""
    img = np.asarray(images)
    V, _, H, W = img.shape
    col = img.transpose(0, 2, 3, 1).reshape(-1, 3)
    pts = np.asarray(points).reshape(-1, 3)
    stat_at = np.flatnonzero(np.asarray(cls).reshape(-1) == 0)[np.asarray(stat_idx)]
    dyn_at = np.flatnonzero(np.asarray(cls)[0].reshape(-1) == 1)[np.asarray(dyn_idx)]
    t = np.asarray(times, np.float32)
    return {"stat_points": pts[stat_at], "stat_colors": col[stat_at], "stat_times": t[stat_at // (H * W)][:, None],
            "dyn_points": pts[dyn_at], "dyn_colors": col[dyn_at], "dyn_times": np.full((len(dyn_at), 1), t[0], np.float32),
            "dyn_coords": np.stack([dyn_at % W, dyn_at // W], 1).astype(np.float32)}
