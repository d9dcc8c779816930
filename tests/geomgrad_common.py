"""Shared by the geometry-gradient fixtures and tests (not a test module).

* ``inputs``: the seeded synthetic tensors of a case (feature maps, collapse weights and biases, probe), drawn with numpy's legacy
  ``RandomState`` -- a generator whose stream is fixed across platforms and versions -- so a fixture stores its seed and shapes, not
  megabytes of weights; ``tests/golden/make_geom_gradients.py`` feeds exactly these to the reference.
* ``box_chain_rule``: a float64 torch restatement of the PER-BOX chain rule the HIP kernel implements
  (``vfa_amd/csrc/vfa_geom_grad.hip``): d vox -> edge gradients from grid_sample's derivative and the area term -> the selected corners
  -> clamp, normalisation, perspective division -> d calib, d grid.  No autograd: the tests compare it with autograd of
  ``oracle/torch_reference``, which pins the formula.
"""
import numpy as np
import torch

SCALE = {"MultiviewC": 1.0, "MultiviewX": 1.0 / 40.0, "Wildtrack": 2.5}


def corner_offsets(cube_size):
    l, w, h = (float(v) for v in cube_size)
    sx = np.array([-1, 1, 1, -1, -1, 1, 1, -1]) * (l / 2)
    sy = np.array([-1, -1, 1, 1, -1, -1, 1, 1]) * (w / 2)
    sz = np.array([0, 0, 0, 0, 1, 1, 1, 1]) * h
    return np.stack([sx, sy, sz], axis=1)


def z_layers(grid_height, cube_size):
    return np.arange(0, grid_height, cube_size[2])


def inputs(seed, n_cams, C, feat_hws, nl, L, W, wscale=3.0, signed=False):
    """-> dict(feats [per scale (n_cams, C, h, w)], weights [(C, C*nl)], biases [(C,)], probe (C, L, W)), all fp32 numpy."""
    rs = np.random.RandomState(seed)
    feats, weights, biases = [], [], []
    for hw in feat_hws:
        f = rs.standard_normal((n_cams, C) + tuple(hw)).astype(np.float32)
        feats.append(f if signed else np.maximum(f, 0).astype(np.float32))
    k = C * nl
    for _ in feat_hws:
        weights.append((rs.uniform(-1, 1, (C, k)) * (wscale / np.sqrt(k))).astype(np.float32))
        biases.append(rs.uniform(-0.3, 0.1, C).astype(np.float32))
    probe = rs.standard_normal((C, L, W)).astype(np.float32)
    return dict(feats=feats, weights=weights, biases=biases, probe=probe)


def _sample(I, x, y):
    """Bilinear sample of I (C,H,W) at normalised points x, y (shape S), align_corners=False, zero padding -> value, d/dx, d/dy (C, S)."""
    C, H, W = I.shape
    X = ((x + 1) * W - 1) / 2
    Y = ((y + 1) * H - 1) / 2
    x0, y0 = torch.floor(X), torch.floor(Y)
    fx, fy = X - x0, Y - y0
    x0, y0 = x0.long(), y0.long()

    def tap(yi, xi):
        ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
        v = I[:, yi.clamp(0, H - 1), xi.clamp(0, W - 1)]
        return v * ok.to(I.dtype)

    nw, ne, sw, se = tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)
    val = (1 - fy) * ((1 - fx) * nw + fx * ne) + fy * ((1 - fx) * sw + fx * se)
    ddx = (W / 2) * ((1 - fy) * (ne - nw) + fy * (se - sw))
    ddy = (H / 2) * ((1 - fx) * (sw - nw) + fx * (se - ne))
    return val, ddx, ddy


def box_chain_rule(feature, calib, grid, zl, co, data, image_size, g_vox, crange=(-1, 0.95)):
    """feature (C,Hf,Wf), calib (3,4), grid (L,W,3), zl (nl), co (8,3), g_vox (L*W, C*nl) = dL/dvox in the reference column order
    c*nl + layer -> (d calib (3,4), d grid (L,W,3)), float64, by the per-box formulas (no autograd)."""
    dt = torch.float64
    feature, calib, grid, zl, co, g_vox = (t.to(dt) for t in (feature, calib, grid, zl, co, g_vox))
    C, Hf, Wf = feature.shape
    L, W = grid.shape[:2]
    nl = zl.numel()
    img_h, img_w = (float(v) for v in image_size)
    pts = grid[None, :, :, None, :] + torch.stack([torch.zeros_like(zl), torch.zeros_like(zl), zl], -1)[:, None, None, None, :]
    pts = pts + co[None, None, None]                                                     # (nl, L, W, 8, 3) grid units
    s = SCALE[data]
    Xw = pts * s
    if data == "Wildtrack":
        Xw = Xw - torch.tensor([300.0, 900.0, 0.0], dtype=dt)
    h = torch.einsum("rj,nlwkj->nlwkr", calib[:, :3], Xw) + calib[:, 3]
    u, v = h[..., 0] / h[..., 2], h[..., 1] / h[..., 2]
    nu_pre, nv_pre = 2 * u / img_w - 1, 2 * v / img_h - 1
    nu, nv = nu_pre.clamp(*crange), nv_pre.clamp(*crange)
    l, r, t, b = nu.min(-1)[0], nu.max(-1)[0], nv.min(-1)[0], nv.max(-1)[0]

    def first(x, m):  # lowest corner index attaining m
        return (x == m[..., None]).to(torch.int64).argmax(-1)

    kl, kr, kt, kb = first(nu, l), first(nu, r), first(nv, t), first(nv, b)
    area = (r - l) * (b - t) * Hf * Wf + 1e-6
    vis = ((area > 1e-6) & (area < Hf * Wf * 0.3)).to(dt)
    I = torch.cumsum(torch.cumsum(feature, -1), -2)
    S = {}
    for name, (x, y) in dict(lt=(l, t), rb=(r, b), rt=(r, t), lb=(l, b)).items():
        S[name] = _sample(I, x.reshape(-1), y.reshape(-1))                               # (C, nl*L*W)
    g = g_vox.view(L * W, C, nl).permute(2, 0, 1).reshape(nl * L * W, C).t()           # (C, nl*L*W), box order (layer, cell)
    N = S["lt"][0] + S["rb"][0] - S["rt"][0] - S["lb"][0]
    ar = area.reshape(-1)
    Q = (g * N).sum(0) / ar
    A = {k: (g * S[k][1]).sum(0) for k in S}
    B = {k: (g * S[k][2]).sum(0) for k in S}
    bh, bw = (b - t).reshape(-1) * Hf * Wf, (r - l).reshape(-1) * Hf * Wf
    vf = vis.reshape(-1)
    dl = ((A["lt"] - A["lb"]) + Q * bh) / ar * vf
    dr = ((A["rb"] - A["rt"]) - Q * bh) / ar * vf
    dtp = ((B["lt"] - B["rt"]) + Q * bw) / ar * vf
    db = ((B["rb"] - B["lb"]) - Q * bw) / ar * vf
    shp = l.shape

    def onehot(k):
        return torch.nn.functional.one_hot(k, 8).to(dt)

    dnu = onehot(kl) * dl.view(shp)[..., None] + onehot(kr) * dr.view(shp)[..., None]
    dnv = onehot(kt) * dtp.view(shp)[..., None] + onehot(kb) * db.view(shp)[..., None]
    dnu = dnu * ((nu_pre >= crange[0]) & (nu_pre <= crange[1])).to(dt)
    dnv = dnv * ((nv_pre >= crange[0]) & (nv_pre <= crange[1])).to(dt)
    du, dv = dnu * 2 / img_w, dnv * 2 / img_h
    h2 = h[..., 2]
    dh = torch.stack([du / h2, dv / h2, -(du * u + dv * v) / h2], -1)                  # (nl, L, W, 8, 3)
    d_calib = torch.zeros(3, 4, dtype=dt)
    d_calib[:, :3] = torch.einsum("nlwkr,nlwkj->rj", dh, Xw)
    d_calib[:, 3] = dh.sum((0, 1, 2, 3))
    dX = torch.einsum("nlwkr,rj->nlwkj", dh, calib[:, :3])
    d_grid = dX.sum((0, 3)) * s
    return d_calib, d_grid
