"""The TSDF integration contract (include/graspqp_hip.h, "scenes from depth images") written in numpy fp64, a small ray caster
that makes its input images, and the layouts the TSDF tests share.  The float32 numbers a kernel is given (grid geometry, poses,
intrinsics, ranges, images) are the inputs; everything after them is float64.  Per node and view, views ascending:
  x_w = R_g (origin + h (i,j,k)) + t_g,  x_c = R_c' (x_w - t_c),  z = x_c.z >= depth_min,  u = fx x_c.x / z + cx (v likewise),
  -0.5 <= u < W - 0.5,  col = floor(u + 0.5),  d = depth[row][col] in [depth_min, depth_max],
  s = trunc for the grid's skipped label, else sdf = d - z >= -trunc and s = min(sdf, trunc),  D = (W D + s) / (W + 1),
  W = min(W + 1, max_weight).
A decision an fp32 kernel cannot be asked to take the oracle's side of marks the node ``ambiguous`` (GUARD_*)."""
import numpy as np

import _clutter_oracle as co

GUARD_PIX = 1e-3   # u + 0.5 or v + 0.5 this close to an integer, within one pixel of the image: the pixel (or in / out) may differ
GUARD_Z = 1e-6     # |z - depth_min| in metres
GUARD_SDF = 1e-6   # |sdf + trunc| in metres: occluded or not
CLEAR = 1e-4       # every pixel's depth stays this clear of depth_min and depth_max


def f32(x):
    return float(np.float32(x))


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """world_from_camera (3,4) float32: the camera at ``eye``, its optical axis (+z) towards ``target``, +x right, +y down."""
    eye, target, up = (np.asarray(a, dtype=np.float64) for a in (eye, target, up))
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return np.concatenate([np.stack([x, y, z], 1), eye[:, None]], 1).astype(np.float32)


def render(cam_T, intrinsics, W, H, plane_z, sphere):
    """Ray-casts the plane z = plane_z (label 0) and the sphere (centre(3), radius) (label 1) from the pose ``cam_T`` (3,4) into a
    z-depth image (H,W) float32 (metres along the optical axis, rounded once; 0 = no hit) and a label image (H,W) int32 (-1 = no hit)."""
    T = np.asarray(cam_T, dtype=np.float64).reshape(3, 4)
    fx, fy, cx, cy = (f32(v) for v in intrinsics)
    col, row = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    dc = np.stack([(col - cx) / fx, (row - cy) / fy, np.ones_like(col)], -1)  # z component 1: the ray parameter IS the z-depth
    dw, o = dc @ T[:, :3].T, T[:, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        sp = (plane_z - o[2]) / dw[..., 2]
    sp = np.where(np.isfinite(sp) & (sp > 0), sp, np.inf)
    c, r = np.asarray(sphere[0], dtype=np.float64), float(sphere[1])
    a, b, q = (dw * dw).sum(-1), (dw * (o - c)).sum(-1), ((o - c) ** 2).sum() - r * r
    disc = b * b - a * q
    with np.errstate(invalid="ignore"):
        ss = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0.0))) / a, np.inf)
    ss = np.where(ss > 0, ss, np.inf)
    depth = np.minimum(sp, ss)
    labels = np.where(ss < sp, 1, 0).astype(np.int32)
    labels[~np.isfinite(depth)] = -1
    return np.where(np.isfinite(depth), depth, 0.0).astype(np.float32), labels


class Volume:
    """Geometry and state of a stack: D and W float64 (G,nx,ny,nz)."""

    def __init__(self, n_grids, shape, origin, voxel, unknown):
        self.out = co.Out(n_grids, shape, origin, voxel)
        self.D = np.full((n_grids,) + self.out.shape, f32(unknown), dtype=np.float64)
        self.W = np.zeros_like(self.D)

    def copy(self):
        v = Volume.__new__(Volume)
        v.out, v.D, v.W = self.out, self.D.copy(), self.W.copy()
        return v


def integrate(vol, depth, labels, cam_T, intrinsics, depth_range, trunc, max_weight=64.0, target_T=None, skip=None):
    """Updates ``vol`` in place; -> info: ``ambiguous`` and ``updated`` (G,nx,ny,nz) bool.  depth (V,H,W) float32, labels (V,H,W)
    int32 or None, cam_T (V,3,4) float32, target_T (G,3,4) float32 or None, skip (G) ints or None."""
    depth = np.asarray(depth, dtype=np.float32)
    depth = depth[None] if depth.ndim == 2 else depth
    V, H, Wd = depth.shape
    if labels is not None:
        labels = np.asarray(labels).reshape(depth.shape)
    cam = np.asarray(cam_T, dtype=np.float32).reshape(V, 3, 4).astype(np.float64)
    fx, fy, cx, cy = (f32(v) for v in intrinsics)
    dmin, dmax, trunc, max_weight = f32(depth_range[0]), f32(depth_range[1]), f32(trunc), f32(max_weight)
    fin = np.isfinite(depth)
    d64 = depth.astype(np.float64)
    assert (np.abs(d64[fin] - dmin) >= CLEAR).all() and (np.abs(d64[fin] - dmax) >= CLEAR).all(), "a depth too close to the range's ends"
    out = vol.out
    xf = out.nodes().numpy()
    G = out.n_grids
    tT = None if target_T is None else np.asarray(target_T, dtype=np.float32).reshape(G, 3, 4).astype(np.float64)
    ambiguous, updated = np.zeros(vol.D.shape, dtype=bool), np.zeros(vol.D.shape, dtype=bool)
    for g in range(G):
        with np.errstate(invalid="ignore", over="ignore"):
            xw = xf if tT is None else xf @ tT[g, :, :3].T + tT[g, :, 3]
        ok_w = np.isfinite(xw).all(-1)
        D, Wt = vol.D[g], vol.W[g]
        D[~ok_w] = np.nan
        sk = -1 if skip is None else int(skip[g])
        for v in range(V):
            with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                xc = (xw - cam[v, :, 3]) @ cam[v, :, :3]  # R' (x - t)
                ok_c = ok_w & np.isfinite(xc).all(-1)
                D[ok_w & ~ok_c] = np.nan
                z = xc[..., 2]
                front = ok_c & (z >= dmin)
                ambiguous[g] |= ok_c & (np.abs(z - dmin) < GUARD_Z)
                zs = np.where(front, z, 1.0)
                u, w = fx * (xc[..., 0] / zs) + cx, fy * (xc[..., 1] / zs) + cy
                inimg = front & (u >= -0.5) & (u < Wd - 0.5) & (w >= -0.5) & (w < H - 0.5)
                near = front & (u >= -1.5) & (u < Wd + 0.5) & (w >= -1.5) & (w < H + 0.5)
                frac = lambda a: np.abs(a + 0.5 - np.round(a + 0.5))
                amb = near & ((frac(u) < GUARD_PIX) | (frac(w) < GUARD_PIX))
            col = np.where(inimg, np.floor(u + 0.5), 0).astype(np.int64)
            row = np.where(inimg, np.floor(w + 0.5), 0).astype(np.int64)
            d = d64[v][row, col]
            with np.errstate(invalid="ignore"):
                valid = inimg & np.isfinite(d) & (d >= dmin) & (d <= dmax)
                carve = valid & (labels[v][row, col] == sk) if (labels is not None and sk >= 0) else np.zeros_like(valid)
                sdf = np.where(valid, d - z, 0.0)
                amb |= valid & ~carve & (np.abs(sdf + trunc) < GUARD_SDF)
                upd = valid & (carve | (sdf >= -trunc))
            s = np.where(carve, trunc, np.minimum(sdf, trunc))
            D[upd] = (Wt[upd] * D[upd] + s[upd]) / (Wt[upd] + 1.0)
            Wt[upd] = np.minimum(Wt[upd] + 1.0, max_weight)
            ambiguous[g] |= amb
            updated[g] |= upd
    return dict(ambiguous=ambiguous, updated=updated)


# ---- the layouts of the GPU and host-body tests ------------------------------------------------------------------------------
TRUNC, DEPTH_RANGE = 0.02, (0.05, 2.0)
IMG_W, IMG_H, INTRINSICS = 40, 32, (45.0, 45.0, 19.63, 15.29)
PLANE_Z, SPHERE = 0.0, ((0.012, -0.007, 0.03), 0.035)
EYES = ((0.30, 0.05, 0.40), (-0.25, 0.20, 0.35), (0.02, -0.33, 0.38), (0.0, 0.01, 0.5))
LOOK = (0.0, 0.0, 0.02)
A_SHAPE, A_ORIGIN, VOXEL = (9, 8, 17), (-0.04, -0.035, -0.04), 0.01  # partial tiles on every axis
B_SHAPE, B_SKIP = (5, 9, 17), (1, -1, 7)


def cameras(n, intrinsics=INTRINSICS, W=IMG_W, H=IMG_H):
    """-> (cam_T (n,3,4) float32, depth (n,H,W) float32, labels (n,H,W) int32) of the first n cameras on the plane-and-sphere scene."""
    T = np.stack([look_at(e, LOOK, up=(0.0, 0.0, 1.0) if abs(e[0]) + abs(e[1]) > 0.05 else (0.0, 1.0, 0.0)) for e in EYES[:n]])
    imgs = [render(t, intrinsics, W, H, PLANE_Z, SPHERE) for t in T]
    return T, np.stack([i[0] for i in imgs]), np.stack([i[1] for i in imgs])


def layout(name):
    """-> (volume, target_T or None, skip or None, n_cameras): "A" one world grid, three cameras; "B" three posed grids, four
    cameras, skip = (1, -1, 7) (grid 0 takes the sphere as free, 7 is a label no pixel carries)."""
    if name == "A":
        return Volume(1, A_SHAPE, A_ORIGIN, VOXEL, -TRUNC), None, None, 3
    T = co.poses(3, 17, 0.02).numpy()
    T[:, :, 3] += np.array([0.0, 0.0, 0.02], dtype=np.float32)  # the grids' centres a few cm about the table top
    return Volume(3, B_SHAPE, co.centred(B_SHAPE, VOXEL), VOXEL, -TRUNC), T, np.array(B_SKIP, dtype=np.int32), 4


def conditions(vol, info, trunc=TRUNC):
    """The fractions the parity tests assert on the oracle's output: (ambiguous, updated by some view, |D| < 0.999 trunc)."""
    fin = np.isfinite(vol.D)
    band = fin & (np.abs(np.where(fin, vol.D, 1.0)) < 0.999 * f32(trunc)) & info["updated"]
    return float(info["ambiguous"].mean()), float(info["updated"].mean()), float(band.mean())


def assert_parity(got_D, got_W, vol, info, tag, caps=True):
    """float32 results against the oracle's state ``vol`` on the non-ambiguous nodes: the weight exactly, D at rtol 1e-5 / atol
    1e-6 (the bound of the same pose chain in the compose tests; the chain rounds by a few 1e-7 m and the running mean adds
    V 6e-8 relative), the NaNs in the same places.  ``caps``: the conditions on the oracle's own output that keep the case from
    passing by leaving nodes out -- at most 5 % ambiguous, at least 50 % updated by some view, at least 10 % inside the band."""
    amb, seen, band = conditions(vol, info)
    print(f"[{tag}] ambiguous {amb:.3%}  seen {seen:.3%}  in band {band:.3%}")
    if caps:
        assert amb <= 0.05 and seen >= 0.50 and band >= 0.10, (tag, amb, seen, band)
    ok = ~info["ambiguous"]
    got_D, got_W = np.asarray(got_D, dtype=np.float64).reshape(vol.D.shape), np.asarray(got_W, dtype=np.float64).reshape(vol.W.shape)
    assert np.array_equal(got_W[ok], vol.W[ok]), tag
    assert np.array_equal(np.isnan(got_D[ok]), np.isnan(vol.D[ok])), tag
    ok &= ~np.isnan(vol.D)
    print(f"[{tag}] max abs err of D {np.abs(got_D[ok] - vol.D[ok]).max():.3e} m on {int(ok.sum())} nodes")
    np.testing.assert_allclose(got_D[ok], vol.D[ok], rtol=1e-5, atol=1e-6, err_msg=tag)
