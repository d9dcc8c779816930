"""Training through the fused lateral producer (``vfa_lateral_convs_train_f32``, ``vfa_lateral_scan_backward_f32``,
``vfa_lateral_conv_backward_f32``; ``vfa_op._LateralIntegrals``; ``VFANet`` with ``FUSE_PRODUCER_TRAIN``) on the MI355X.

The forward is pinned bit for bit to the inference kernels, dz bit for bit to the masked ``integral_image_backward``, and the
parameter / trunk gradients are measured against a float64 autograd composition (conv2d -> group_norm -> the fp32 forward's mask ->
cumsum . cumsum), next to the fp32 library composition with the same mask (MIOpen conv + torch GroupNorm autograd).
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = torch.device("cuda:0")
EPS = 1e-5

BENCH = dict(n=7, maps=((128, 90, 160), (256, 45, 80), (512, 23, 40)))
RAGGED = dict(n=1, maps=((128, 13, 19), (256, 7, 10), (512, 4, 5)))


def _branches(n, maps, seed, bias_offset=0.0):
    """Synthetic trunk maps and lateral parameters: [(feat, weight (256,K), bias, gamma, beta)] on the device.  ``bias_offset``: added
    to every channel's conv bias, so every group's mean moves by it while its spread stays (|mu| >> sigma)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for K, h, w in maps:
        feat = torch.relu(torch.randn(n, K, h, w, generator=g))
        wt = torch.randn(256, K, generator=g) / K ** 0.5
        b = torch.randn(256, generator=g) * 0.5 + bias_offset
        gam = torch.rand(256, generator=g) + 0.5
        bet = torch.randn(256, generator=g) * 0.3
        out.append(tuple(t.to(DEV) for t in (feat, wt, b, gam, bet)))
    return out


def _golden_branches(name):
    d = np.load(os.path.join(GOLDEN, name))
    return [tuple(torch.from_numpy(np.ascontiguousarray(d[f"{k}{s}"])).float().to(DEV) for k in ("feat", "latw", "latb", "gnw", "gnb"))
            for s in (8, 16, 32)], float(d["gn_eps"])


CASES = {
    "bench": lambda: (_branches(BENCH["n"], BENCH["maps"], 1), EPS),
    "ragged": lambda: (_branches(RAGGED["n"], RAGGED["maps"], 2), EPS),
    "one_map": lambda: (_branches(2, ((256, 21, 33),), 3), EPS),
    "two_maps": lambda: (_branches(3, ((128, 17, 24), (512, 5, 9)), 4), EPS),
    "golden_mc": lambda: _golden_branches("laterals_mc.npz"),
    "golden_mc_nl1": lambda: _golden_branches("laterals_mc_nl1.npz"),
}


def _node(branches, eps, grad=True):
    """The producer node on leaf copies of the inputs -> (integrals, leaves)."""
    from vfa_amd import vfa_op
    leaves = [[t.detach().clone().requires_grad_(grad) for t in br] for br in branches]
    ns = len(leaves)
    tensors = [l[0] for l in leaves] + [l[1] for l in leaves] + [l[2] for l in leaves] + [l[3] for l in leaves] + [l[4] for l in leaves]
    outs = vfa_op._LateralIntegrals.apply(tuple(eps for _ in range(ns)), *tensors)
    return outs[:ns], outs[ns:], leaves


def _probes(integrals, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return [torch.randn(i.shape, generator=g, device=DEV) for i in integrals]


@pytest.mark.parametrize("case", sorted(CASES))
def test_training_forward_is_the_inference_forward(case):
    """y, scale, shift bit for bit ``vfa_lateral_convs_f32``; the node's integral images bit for bit the inference producer's; mean and
    rstd the float64 statistics of y."""
    from vfa_amd import ops
    branches, eps = CASES[case]()
    args = [(f, w, b, g, be, eps) for f, w, b, g, be in branches]
    inf = ops.lateral_convs(args)
    inf = [tuple(t.clone() for t in p) for p in inf]
    tr = ops.lateral_convs_train(args)
    for (y0, s0, h0), (y1, s1, h1, mu, rs) in zip(inf, tr):
        for a, b in ((y0, y1), (s0, s1), (h0, h1)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        n, h, w, _ = y1.shape
        yg = y1.double().reshape(n, h * w, 16, 16)
        m64 = yg.mean(dim=(1, 3))
        v64 = ((yg - m64[:, None, :, None]) ** 2).mean(dim=(1, 3))
        torch.testing.assert_close(mu, m64, rtol=1e-12, atol=1e-12 * float(yg.abs().max()))
        torch.testing.assert_close(rs, 1.0 / torch.sqrt(v64 + eps), rtol=1e-9, atol=0)
    want = ops.integral_images([p[0] for p in inf], [p[1] for p in inf], [p[2] for p in inf], channels_last=True)
    got, absmax, _ = _node(branches, eps)
    for a, b, sa, sb in zip(want, got, want.absmax, absmax):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert torch.equal(sa, sb) and not sb.requires_grad


@pytest.mark.parametrize("case", ["bench", "ragged", "two_maps"])
def test_dz_is_the_masked_integral_image_backward(case):
    """dz == integral_image_backward(d integral), channels-last, times [y * scale + shift > 0], bit for bit; garbage in the border of
    d integral changes nothing."""
    from vfa_amd import ops
    branches, eps = CASES[case]()
    tr = ops.lateral_convs_train([(f, w, b, g, be, eps) for f, w, b, g, be in branches])
    ys, scs, shs, mus, rss = (list(t) for t in zip(*tr))
    gis = _probes([torch.empty(y.shape[0], y.shape[1] + 2, y.shape[2] + 2, 256) for y in ys], 7)
    Ks = [br[0].shape[1] for br in branches]
    gammas = [br[3] for br in branches]
    dzs = ops.lateral_scan_backward([g.clone() for g in gis], ys, scs, shs, mus, rss, gammas, Ks)[0]
    dzs = [d.clone() for d in dzs]
    for g, y, sc, sh, dz in zip(gis, ys, scs, shs, dzs):
        ref = ops.integral_image_backward(g.clone()).permute(0, 2, 3, 1)
        t = y * sc[:, None, None, :]
        t = t + sh[:, None, None, :]
        ref = torch.where(t > 0, ref, torch.zeros_like(ref))
        assert torch.equal(ref.contiguous().view(torch.int32), dz.view(torch.int32))
        assert 0.05 < (t > 0).float().mean() < 0.95
    dirty = []
    for g in gis:
        d = g.clone()
        d[:, 0] = 1e30
        d[:, -1] = float("nan")
        d[:, :, 0] = -3e7
        d[:, :, -1] = float("inf")
        dirty.append(d)
    dz2 = ops.lateral_scan_backward(dirty, ys, scs, shs, mus, rss, gammas, Ks)[0]
    for a, b in zip(dzs, dz2):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def _reference_grads(branches, eps, probes, masks, dtype):
    """conv2d -> group_norm -> the forward's mask -> cumsum . cumsum -> (integral * probe).sum(), autograd in ``dtype``."""
    leaves = [[t.detach().to(dtype).clone().requires_grad_(True) for t in br] for br in branches]
    loss = 0
    for (f, w, b, g, be), p, m in zip(leaves, probes, masks):
        y = F.conv2d(f, w[:, :, None, None], b)
        z = F.group_norm(y, 16, g, be, eps)
        a = z * m.permute(0, 3, 1, 2).to(dtype)
        integ = F.pad(a.cumsum(-1).cumsum(-2), (1, 1, 1, 1)).permute(0, 2, 3, 1)
        loss = loss + (integ * p.to(dtype)).sum()
    loss.backward()
    return [[t.grad for t in l] for l in leaves]


def _rel(a, ref):
    return float((a.double() - ref).norm() / ref.norm().clamp_min(1e-300))


LARGE_MEAN = 3e4  # group mean / spread ~ 4e4: fp32 (y - mu) would lose ~1e-3 of sigma (ulp(3e4) = 2^-9)


def _group_mean_over_sigma(y):
    n, h, w, _ = y.shape
    yg = y.double().reshape(n, h * w, 16, 16)
    return float((yg.mean(dim=(1, 3)).abs() / yg.std(dim=(1, 3), unbiased=False)).min())


@pytest.mark.parametrize("case", ["bench", "ragged", "one_map", "two_maps", "golden_mc", "golden_mc_nl1", "large_mean"])
def test_gradients_against_float64(case):
    """d f, d W, d b, d gamma, d beta of the HIP backward: normwise no further from float64 than 2x the fp32 library composition (with
    the same mask), with a floor of 2e-6."""
    from vfa_amd import ops
    if case == "large_mean":
        branches, eps = _branches(2, ((128, 16, 22), (256, 8, 11)), 5, bias_offset=LARGE_MEAN), EPS
    else:
        branches, eps = CASES[case]()
    integrals, _, leaves = _node(branches, eps)
    probes = _probes(integrals, 11)
    loss = sum((i * p).sum() for i, p in zip(integrals, probes))
    loss.backward()
    tr = ops.lateral_convs_train([(f, w, b, g, be, eps) for f, w, b, g, be in branches])
    masks = []
    for y, sc, sh, *_ in tr:
        t = y * sc[:, None, None, :]
        t = t + sh[:, None, None, :]
        masks.append((t > 0).float())
    if case == "large_mean":
        assert min(_group_mean_over_sigma(t[0]) for t in tr) >= 1e3
    ref = _reference_grads(branches, eps, probes, masks, torch.float64)
    lib = _reference_grads(branches, eps, probes, masks, torch.float32)
    floor = 2e-6
    names = ("feat", "weight", "bias", "gamma", "beta")
    worst = []
    for k, (l, r, lb) in enumerate(zip(leaves, ref, lib)):
        for name, t, rr, ll in zip(names, l, r, lb):
            e_hip, e_lib = _rel(t.grad.reshape(rr.shape), rr), _rel(ll, rr)
            worst.append((name, k, e_hip, e_lib))
            assert e_hip <= 2 * max(e_lib, floor), (case, name, k, e_hip, e_lib)
    print(case, " ".join(f"{n}{k}: {eh:.2e} (lib {el:.2e})" for n, k, eh, el in worst))


def test_backward_around_a_large_group_mean():
    """|mu| / sigma >= 1e3 in every group: the backward taken from the forward's own y (float64 GroupNorm, the fp32 forward's mask, the
    cumsums and the 1x1 convolution's two products in float64) against the HIP gradients.  The fp32 y is the input here, so what is
    measured is the backward's own arithmetic: S2 and d y formed around the mean stay within 3e-6.  (y - mu) or S2 formed in fp32
    would be off by ~1e-3 of sigma in every element: ~1e-5 in d f / d W and ~1e-3 in d gamma.)"""
    from vfa_amd import ops
    branches = _branches(2, ((128, 16, 22), (256, 8, 11)), 5, bias_offset=LARGE_MEAN)
    integrals, _, leaves = _node(branches, EPS)
    probes = _probes(integrals, 13)
    sum((i * p).sum() for i, p in zip(integrals, probes)).backward()
    tr = ops.lateral_convs_train([(f, w, b, g, be, EPS) for f, w, b, g, be in branches])
    for (y, sc, sh, *_), (f, w, b, g, be), l, p in zip(tr, branches, leaves, probes):
        assert _group_mean_over_sigma(y) >= 1e3
        t = y * sc[:, None, None, :]
        t = t + sh[:, None, None, :]
        mask = (t > 0).double().permute(0, 3, 1, 2)
        y64 = y.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        g64, be64 = g.double().requires_grad_(True), be.double().requires_grad_(True)
        a = F.group_norm(y64, 16, g64, be64, EPS) * mask
        integ = F.pad(a.cumsum(-1).cumsum(-2), (1, 1, 1, 1)).permute(0, 2, 3, 1)
        (integ * p.double()).sum().backward()
        dy = y64.grad
        want = {"feat": torch.einsum("ck,nchw->nkhw", w.double(), dy), "weight": torch.einsum("nchw,nkhw->ck", dy, f.double()),
                "bias": dy.sum(dim=(0, 2, 3)), "gamma": g64.grad, "beta": be64.grad}
        errs = {k: _rel(t_.grad.reshape(want[k].shape), want[k]) for k, t_ in zip(("feat", "weight", "bias", "gamma", "beta"), l)}
        print("large mean", {k: f"{e:.1e}" for k, e in errs.items()})
        assert max(errs.values()) <= 3e-6, errs


@pytest.mark.parametrize("frozen", ["trunk", "parameters"])
def test_subsets_of_needs_input_grad(frozen):
    """A frozen trunk runs no d f product.  Frozen conv / GroupNorm parameters get no gradient, a frozen conv weight costs no d W
    product, and d beta is not written when no beta wants it.  Every other gradient is the all-trainable run's, bit for bit."""
    from vfa_amd import ops, vfa_op
    branches, eps = CASES["ragged"]()
    full, _, leaves_full = _node(branches, eps)
    probes = _probes(full, 3)
    sum((i * p).sum() for i, p in zip(full, probes)).backward()

    leaves = [[t.detach().clone().requires_grad_(True) for t in br] for br in branches]
    if frozen == "trunk":
        for l in leaves:
            l[0].requires_grad_(False)
    else:  # conv weight of map 0, conv bias of map 2, gamma of map 1, every beta
        for k, j in ((0, 1), (2, 2), (1, 3), (0, 4), (1, 4), (2, 4)):
            leaves[k][j].requires_grad_(False)
    ns = len(leaves)
    tensors = [l[0] for l in leaves] + [l[j] for j in range(1, 5) for l in leaves]
    with ops.KernelTimer() as kt:
        outs = vfa_op._LateralIntegrals.apply(tuple(eps for _ in range(ns)), *tensors)
        sum((i * p).sum() for i, p in zip(outs[:ns], probes)).backward()
    torch.cuda.synchronize()
    conv_tags = list(kt.summary()["vfa_lateral_conv_backward_f32"]["by_tag"])  # (n, Ks, hws, want_feat, want_weight)
    scan_tags = list(kt.summary()["vfa_lateral_scan_backward_f32"]["by_tag"])  # (n, Ks, hws, want (bias, gamma, beta))
    if frozen == "trunk":
        assert [(t[3], t[4]) for t in conv_tags] == [((False,) * 3, (True,) * 3)], conv_tags
        assert [t[3] for t in scan_tags] == [(True, True, True)], scan_tags
    else:
        assert [(t[3], t[4]) for t in conv_tags] == [((True,) * 3, (False, True, True))], conv_tags
        assert [t[3] for t in scan_tags] == [(True, True, False)], scan_tags
    for l, lf in zip(leaves, leaves_full):
        for t, tf in zip(l, lf):
            if t.requires_grad:
                assert torch.equal(t.grad.view(torch.int32), tf.grad.view(torch.int32))
            else:
                assert t.grad is None


def test_only_calibs_require_grad_runs_no_producer_backward():
    """A frozen network with only the camera matrices requiring grad: the producer's backward never runs, and d calibs agrees with the
    switch-off run (the laterals come from another convolution there: not bitwise)."""
    net, images, calibs, grid = _small_net(nl=1)
    for p in net.parameters():
        p.requires_grad_(False)
    got = {}
    for on in (True, False):
        c = calibs.clone().requires_grad_(True)
        with _switch(on), _kernels() as kt:
            out = net.ortho_features(images, c, grid)
            (out * _probe_like(out)).sum().backward()
        torch.cuda.synchronize()
        ran = set(kt.summary())
        assert "vfa_lateral_scan_backward_f32" not in ran and "vfa_lateral_conv_backward_f32" not in ran, sorted(ran)
        if on:
            assert "vfa_lateral_convs_train_f32" in ran, sorted(ran)
        got[on] = c.grad
    assert got[True].abs().max() > 0
    torch.testing.assert_close(got[True], got[False], rtol=2e-3, atol=2e-3 * float(got[False].abs().max()))


@pytest.mark.parametrize("deterministic", [False, True])
def test_backward_is_bit_reproducible(deterministic):
    branches, eps = CASES["bench"]()
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(deterministic, warn_only=True)
    try:
        runs = []
        for _ in range(2):
            integrals, _, leaves = _node(branches, eps)
            probes = _probes(integrals, 5)
            sum((i * p).sum() for i, p in zip(integrals, probes)).backward()
            runs.append([t.grad.clone() for l in leaves for t in l])
        for a, b in zip(*runs):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    finally:
        torch.use_deterministic_algorithms(prev)


# ---- end to end: VFANet with the switch on --------------------------------------------------------------------------------------
class _switch:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from vfa_amd import vfanet
        self.prev = vfanet.FUSE_PRODUCER_TRAIN
        vfanet.FUSE_PRODUCER_TRAIN = self.on

    def __exit__(self, *exc):
        from vfa_amd import vfanet
        vfanet.FUSE_PRODUCER_TRAIN = self.prev


def _kernels():
    from vfa_amd import ops
    return ops.KernelTimer()


def _probe_like(t):
    g = torch.Generator(device=t.device).manual_seed(9)
    return torch.randn(t.shape, generator=g, device=t.device)


def _small_net(nl):
    import vfa_amd
    from types import SimpleNamespace
    from vfa_amd.vfanet import VFANet
    from vfa_amd.synthetic import ring_cameras
    torch.manual_seed(0)
    args = SimpleNamespace(data="MultiviewC", image_size=(128, 192))
    net = VFANet(args, grid_height=64 if nl > 1 else 32, cube_size=(50, 50, 32), angle_range=12).to(DEV).train()
    images = torch.rand(2, 3, 128, 192, device=DEV)
    calibs = ring_cameras(2, (400., 300., 0.), 1100., 400., 160., (192, 128)).to(DEV)
    grid = vfa_amd.make_grid((600, 800), cube_LW=(50, 50), dataset="MultiviewC").to(DEV)[None]
    assert net.vfa8.num_grid_layer == nl
    return net, images, calibs, grid


class _SameForward(torch.autograd.Function):
    """Forward: the HIP producer's own lateral map relu(y * scale + shift) (NCHW); backward: the incoming gradient times that map's
    ReLU mask, handed to the library's pre-activation (MIOpen conv + torch GroupNorm)."""

    @staticmethod
    def forward(ctx, pre, lat, mask):
        ctx.save_for_backward(mask)
        return lat.clone()

    @staticmethod
    def backward(ctx, g):
        (mask,) = ctx.saved_tensors
        return g * mask, None, None


def _laterals_with_the_producers_forward(net):
    """``laterals()`` whose forward values are the HIP producer's bit for bit (so the frame node sees the very integral images of the
    switch-on step) and whose backward is the library's: torch GroupNorm and MIOpen conv autograd under the producer's mask."""
    from vfa_amd import ops
    convs, norms = (net.lat8, net.lat16, net.lat32), (net.bn8, net.bn16, net.bn32)

    def laterals(images):
        x = (images - net.mean.view(3, 1, 1)) / net.std.view(3, 1, 1)
        feats = net.base(x)
        with torch.no_grad():
            parts = ops.lateral_convs([(f, c.weight, c.bias, g.weight, g.bias, g.eps) for f, c, g in zip(feats, convs, norms)])
        out = []
        for f, c, g, (y, sc, sh) in zip(feats, convs, norms, parts):
            t = y * sc[:, None, None, :]
            t = t + sh[:, None, None, :]  # (the row scan's two fp32 operations)
            lat = torch.relu(t).permute(0, 3, 1, 2).contiguous()
            mask = (t > 0).float().permute(0, 3, 1, 2).contiguous()
            out.append(_SameForward.apply(g(c(f)), lat, mask))
        return tuple(out)
    return laterals


@pytest.mark.parametrize("nl", [1, 2])
def test_vfanet_trains_through_the_producer(nl):
    """Switch on: the training step runs the new entry points and neither vfa_integral_images_f32 nor vfa_integral_image_backward_f32,
    and a few SGD steps lower the loss.  Against a switch-off step whose lateral maps carry the producer's forward values (frame node,
    heads and trunk are then the same computation; only the producer's backward differs: HIP against torch GroupNorm + MIOpen conv
    autograd).  With float atomics two steps of the SAME path are not bit-identical (the frame node's scatter into d integral), and box sums -- differences
    of large integral-image values -- amplify such 1e-7 differences to 1e-5..1e-3 of the map on tiny maps (tests/test_lateral.py, the
    library-lateral margin).  Under torch's deterministic switch the spread is 0 and the steps agree to ~2e-6: the bound is 1e-5, or
    10x the switch-on step's own run-to-run spread should that ever be larger."""
    net, images, calibs, grid = _small_net(nl)
    state = {k: v.clone() for k, v in net.state_dict().items()}
    target = torch.rand(1, 1, grid.shape[1], grid.shape[2], device=DEV)

    def step():
        net.zero_grad()
        out = net(images, calibs, grid)
        loss = ((out["heatmap"] - target) ** 2).mean() + 1e-3 * out["loc_offset"].pow(2).mean()
        loss.backward()
        return loss

    # (deterministic mode: the frame node's scatter into d integral adds in a fixed order -- with float atomics its order, and the bits
    # of everything the reverse cumsums make of it, change from step to step)
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    grads = {}
    for on in (False, True, "again"):
        net.load_state_dict(state)
        if not on:
            net.laterals = _laterals_with_the_producers_forward(net)
        try:
            with _switch(bool(on)), _kernels() as kt:
                step()
            torch.cuda.synchronize()
        finally:
            if not on:
                del net.laterals
        ran = set(kt.summary())
        if on is True:
            for name in ("vfa_lateral_convs_train_f32", "vfa_integral_images_hwc_f32", "vfa_lateral_scan_backward_f32",
                         "vfa_lateral_conv_backward_f32"):
                assert name in ran, (name, sorted(ran))
            assert "vfa_integral_images_f32" not in ran and "vfa_integral_image_backward_f32" not in ran, sorted(ran)
        elif not on:
            assert "vfa_lateral_scan_backward_f32" not in ran and "vfa_integral_image_backward_f32" in ran, sorted(ran)
        grads[on] = {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}
    torch.use_deterministic_algorithms(prev)

    def rel(a, b):
        return float((a - b).norm() / b.norm().clamp_min(1e-30))
    names = [k for k in grads[False] if k.startswith(("lat", "bn8", "bn16", "bn32", "base.", "vfa"))]
    errs = {k: rel(grads[True][k], grads[False][k]) for k in names}
    spread = max(rel(grads["again"][k], grads[True][k]) for k in names)
    print(f"nl={nl} run-to-run spread {spread:.1e};", " ".join(f"{k}: {e:.1e}" for k, e in sorted(errs.items(), key=lambda kv: -kv[1])[:10]))
    assert len(errs) >= 20
    assert max(errs.values()) <= max(10 * spread, 1e-5), (spread, errs)

    net.load_state_dict(state)
    opt = torch.optim.SGD(net.parameters(), lr=1e-3, momentum=0.9)
    losses = []
    with _switch(True):
        for _ in range(5):
            opt.zero_grad()
            loss = step()
            opt.step()
            losses.append(loss.item())
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses


def test_frames_and_camera_sharding_route_through_the_producer():
    """Switch on, a (B, N, ...) batch with gradients runs the producer node frame by frame: its map is the per-frame maps and its
    gradients the sum of the per-frame steps.  ``distributed=True`` (no process group: this rank holds every camera) runs the same
    node and gives the same map and gradients.  (Within 1e-3: two passes of the trunk are not bit-identical, and the box sums
    amplify that; see test_vfanet_trains_through_the_producer.)"""
    net, images, calibs, grid = _small_net(nl=1)
    frames = torch.stack([images, images.flip(-1)])
    params = [p for p in net.parameters()]

    def grads_of(fn):
        net.zero_grad()
        with _switch(True), _kernels() as kt:
            out = fn()
        torch.cuda.synchronize()
        return out, [None if p.grad is None else p.grad.clone() for p in params], kt.summary()

    probe = torch.randn(2, 256, grid.shape[1], grid.shape[2], generator=torch.Generator(device=DEV).manual_seed(4), device=DEV)

    def batched():
        out = net.ortho_features(frames, calibs, grid)
        (out * probe).sum().backward()
        return out.detach()

    def per_frame():
        outs = []
        for b in range(2):
            o = net.ortho_features(frames[b], calibs, grid)
            (o * probe[b:b + 1]).sum().backward()
            outs.append(o.detach())
        return torch.cat(outs)

    out_b, g_b, ran_b = grads_of(batched)
    out_f, g_f, _ = grads_of(per_frame)
    assert ran_b["vfa_lateral_scan_backward_f32"]["launches"] == 2 and ran_b["vfa_lateral_conv_backward_f32"]["launches"] == 2
    assert "vfa_integral_image_backward_f32" not in ran_b
    assert float((out_b - out_f).abs().max()) <= 1e-3 * float(out_f.abs().max())
    checked = 0
    for a, b in zip(g_b, g_f):
        if b is not None and b.abs().max() > 0:
            assert float((a - b).norm() / b.norm()) <= 1e-3
            checked += 1
    assert checked >= 20

    def sharded(distributed):
        def fn():
            out = net.ortho_features(images, calibs, grid, distributed=distributed)
            (out * probe[:1]).sum().backward()
            return out.detach()
        return fn

    out_d, g_d, ran_d = grads_of(sharded(True))
    out_s, g_s, _ = grads_of(sharded(False))
    assert "vfa_lateral_scan_backward_f32" in ran_d and "vfa_integral_image_backward_f32" not in ran_d
    assert float((out_d - out_s).abs().max()) <= 1e-3 * float(out_s.abs().max())
    for a, b in zip(g_d, g_s):
        if b is not None and b.abs().max() > 0:
            assert float((a - b).norm() / b.norm()) <= 1e-3
