"""Max-over-cameras fusion (``view_reduce="max"``) on the MI355X.

Contract: t_v = (relu(lin8_v + b8) + relu(lin16_v + b16)) + relu(lin32_v + b32) in fp32, ortho = max over v of t_v (torch.stack(...).max(0)),
each element's gradient to the lowest camera attaining the maximum, through that camera's ReLU masks.  Ground truth: the kernels against
torch on random pre-activations (bitwise), the path against ``oracle.torch_reference.vfa_forward`` per camera and scale composed with
``torch.stack(...).max(0)`` on the VFANet fixtures (fp32 and float64).  -m gpu.
"""
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import VFANET_CASES, golden_path
from geomgrad_common import corner_offsets, z_layers

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


def _torch_max(lins, biases):
    t = [(torch.relu(l8 + biases[0]) + torch.relu(l16 + biases[1])) + torch.relu(l32 + biases[2]) for l8, l16, l32 in zip(*lins)]
    return torch.stack(t).max(0)


def _random_lins(n, M, N, seed, dev):
    g = torch.Generator().manual_seed(seed)
    lins = [torch.randn((n, M, N), generator=g).to(dev) for _ in range(3)]
    biases = [(0.3 * torch.randn(N, generator=g)).to(dev) for _ in range(3)]
    return lins, biases


@pytest.mark.parametrize("n", [1, 2, 7, 32])
@pytest.mark.parametrize("N", [8, 256])
def test_kernels_match_torch_bitwise(n, N):
    from vfa_amd import _lib, ops
    dev = _dev()
    M = 37 if N == 256 else 1001  # ragged: no multiple of a workgroup's elements
    lins, biases = _random_lins(n, M, N, 100 * n + N, dev)
    out, argmax = ops.scale_view_max(*lins, *biases)
    want = _torch_max(lins, biases)
    assert torch.equal(out, want.values) and torch.equal(argmax.long(), want.indices)
    # backward: torch autograd through the same composition
    probe = torch.randn((M, N), generator=torch.Generator().manual_seed(3)).to(dev)
    ref = [l.clone().requires_grad_(True) for l in lins] + [b.clone().requires_grad_(True) for b in biases]
    (_torch_max(ref[:3], ref[3:]).values * probe).sum().backward()
    got = ops.scale_view_max_backward(probe, *lins, *biases, argmax)
    for k in range(3):
        assert torch.equal(got[k], ref[k].grad), f"grad_lin{k}"
        torch.testing.assert_close(got[3 + k], ref[3 + k].grad, rtol=1e-5, atol=1e-5 * float(ref[3 + k].grad.abs().max()))
    again = ops.scale_view_max_backward(probe, *lins, *biases, argmax)
    for a, b in zip(got, again):
        assert torch.equal(a, b)
    # the C entry point's own bias sums (vfa_column_sum_f32 over the dense rows): the same value within rounding
    glins = [torch.empty_like(lins[0]) for _ in range(3)]
    gb = [torch.empty(N, device=dev) for _ in range(3)]
    _lib.call("vfa_scale_view_max_backward_f32", _lib.ptr(probe), *(_lib.ptr(x) for x in lins), *(_lib.ptr(b) for b in biases),
              _lib.ptr(argmax), *(_lib.ptr(g) for g in glins), *(_lib.ptr(b) for b in gb), n, M, N, _lib.current_stream_handle())
    for k in range(3):
        assert torch.equal(glins[k], got[k])
        torch.testing.assert_close(gb[k], got[3 + k], rtol=1e-5, atol=1e-5 * float(got[3 + k].abs().max()))
    if N == 8:  # the one-channel kernels: N not a multiple of 4
        l2, b2 = _random_lins(n, 33, 7, 9, dev)
        o2, a2 = ops.scale_view_max(*l2, *b2)
        w2 = _torch_max(l2, b2)
        assert torch.equal(o2, w2.values) and torch.equal(a2.long(), w2.indices)
        p2 = torch.randn((33, 7), generator=torch.Generator().manual_seed(8)).to(dev)
        r2 = [l.clone().requires_grad_(True) for l in l2]
        (_torch_max(r2, b2).values * p2).sum().backward()
        g2 = ops.scale_view_max_backward(p2, *l2, *b2, a2)
        for k in range(3):
            assert torch.equal(g2[k], r2[k].grad)


def test_ties_go_to_the_first_camera_and_nan_propagates():
    from vfa_amd import ops
    dev = _dev()
    n, M, N = 5, 64, 256
    lins, biases = _random_lins(n, M, N, 7, dev)
    for l in lins:
        l[:, :16] = l[0, :16]  # rows 0-15: every camera identical -> exact ties
        l[3, 16:32] = l[1, 16:32]  # rows 16-31: cameras 1 and 3 identical
    lins[0][4, 40, 5] = float("nan")
    lins[1][2, 41, 6] = float("nan")
    lins[2][3, 41, 6] = float("nan")
    out, argmax = ops.scale_view_max(*lins, *biases)
    want = _torch_max(lins, biases)
    assert (argmax[:16] == 0).all()
    assert bool(torch.isnan(out[40, 5])) and int(argmax[40, 5]) == 4
    assert bool(torch.isnan(out[41, 6])) and int(argmax[41, 6]) == 2  # the first NaN camera wins
    assert torch.equal(argmax.long(), want.indices)
    assert torch.equal(torch.nan_to_num(out, nan=-1.0), torch.nan_to_num(want.values, nan=-1.0))
    probe = torch.ones((M, N), device=dev)
    g = ops.scale_view_max_backward(probe, *lins, *biases, argmax)
    tie = argmax[16:32] == 1
    for k in range(3):
        assert not g[k][1:, :16].any()  # exact ties: the other cameras get exactly zero
        assert not g[k][3, 16:32][tie].any()


def _load(name):
    z = np.load(golden_path(name), allow_pickle=False)
    return {k: z[k] for k in z.files}


def _mods(d, dev):
    import vfa_amd
    args = SimpleNamespace(data=str(d["data"]), image_size=tuple(int(v) for v in d["image_size"]))
    mods = []
    for s in (8, 16, 32):
        m = vfa_amd.VFA(256, grid_height=float(d["grid_height"]), cube_size=tuple(float(v) for v in d["cube_size"]), args=args).to(dev)
        with torch.no_grad():
            m.collapse.weight.copy_(torch.from_numpy(d[f"weight{s}"]))
            m.collapse.bias.copy_(torch.from_numpy(d[f"bias{s}"]))
        mods.append(m)
    return mods


def _oracle_max(d, dtype, grad=False):
    """The reference's per-camera maps (oracle.torch_reference.vfa_forward per camera and scale, vfanet.py:79) composed with
    torch.stack(...).max(0), on the CPU in ``dtype``.  -> (ortho (C,L,W), leaves dict)."""
    from oracle import torch_reference as tr
    leaves = {f"lat{s}": torch.from_numpy(d[f"lat{s}"]).to(dtype) for s in (8, 16, 32)}
    leaves.update({f"weight{s}": torch.from_numpy(d[f"weight{s}"]).to(dtype) for s in (8, 16, 32)})
    leaves.update({f"bias{s}": torch.from_numpy(d[f"bias{s}"]).to(dtype) for s in (8, 16, 32)})
    leaves["calibs"] = torch.from_numpy(d["calibs"]).to(dtype)
    leaves["grid"] = torch.from_numpy(d["grid"]).to(dtype)
    if grad:
        for v in leaves.values():
            v.requires_grad_(True)
    zl = torch.from_numpy(z_layers(float(d["grid_height"]), d["cube_size"])).to(dtype)
    co = torch.from_numpy(corner_offsets(d["cube_size"])).to(dtype)
    data, image_size = str(d["data"]), tuple(int(v) for v in d["image_size"])
    per_cam = []
    for cam in range(d["calibs"].shape[0]):
        f = [tr.vfa_forward(leaves[f"lat{s}"][cam:cam + 1], leaves["calibs"][cam], leaves["grid"], leaves[f"weight{s}"],
                            leaves[f"bias{s}"], zl, co, data, image_size) for s in (8, 16, 32)]
        per_cam.append((f[0] + f[1] + f[2])[0])
    stacked = torch.stack(per_cam)
    return (stacked.max(0).values, leaves, stacked.detach()) if grad else (stacked.max(0).values, leaves)


def _tol(ref):
    return dict(rtol=1e-4, atol=1e-5 * float(np.abs(ref).max()))


@pytest.mark.parametrize("name", VFANET_CASES)
def test_aggregate_max_matches_the_oracle_composition(name):
    import vfa_amd
    dev = _dev()
    d = _load(name)
    mods = _mods(d, dev)
    lats = [torch.from_numpy(d[f"lat{s}"]).to(dev) for s in (8, 16, 32)]
    calibs, grid = torch.from_numpy(d["calibs"]).to(dev), torch.from_numpy(d["grid"])[None].to(dev)
    with torch.no_grad():
        out = vfa_amd.aggregate_views(*mods, *lats, calibs, grid, view_reduce="max")
        summed = vfa_amd.aggregate_views(*mods, *lats, calibs, grid)
    ref32, _ = _oracle_max(d, torch.float32)
    ref64, _ = _oracle_max(d, torch.float64)
    got = out[0].cpu().numpy()
    assert np.abs(ref64.numpy()).max() > 0
    np.testing.assert_allclose(got, ref32.numpy(), **_tol(ref32.numpy()))
    # against float64: no farther than the reference's own fp32 composition (its integral images round at ~1e-4 of the map)
    e64, n64 = _rel(got, ref64.numpy()), _rel(ref32.numpy(), ref64.numpy())
    print(f"[view max] {name}: |hip - float64| {e64:.2e}, |fp32 oracle - float64| {n64:.2e}")
    assert e64 <= 1.5 * n64 + 1e-5
    assert not torch.allclose(summed, out)  # three cameras: the max is not the sum


def _rel(a, b):
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max() / max(np.abs(b).max(), 1e-30))


@pytest.mark.parametrize("name", ["vfanet_mc.npz", "vfanet_mc_nl1.npz", "vfanet_wt_nl1.npz"])
def test_max_gradients_vs_float64_autograd(name):
    """d lat*, d weight*, d bias*, d calibs, d grid of ``(ortho * probe).sum()`` against autograd of the oracle composition in float64,
    within the limits of tests/test_geometry_gradients.py for every tensor: max|hip - g32| <= max(floor, 2 n) and max|hip - g64| <=
    1.5 n + floor, n = max|g32 - g64| / max|g64| measured from the composition's own fp32 run, floor 5e-5 for the features, 2e-5 for
    weights and biases (tests/test_reference_gradients.py) and 5e-4 for calibs and grid.  k = 2 against fp32: the HIP sums and the
    oracle's fp32 sums are two independent roundings of the float64 value (on vfanet_mc_nl1 d weight8 the HIP result is 5x closer to
    float64 than the fp32 oracle is).  The geometry floor is 5x that of tests/test_geometry_gradients.py: under the maximum a cell's
    calib / grid gradient comes from its winning camera alone, so the integral images' rounding and the ReLU masks of pre-activations
    within the product's rounding of zero are not averaged over the cameras as in the sum (measured: 4.9e-4 of max|g64| for d grid
    on vfanet_mc_nl1, n = 1.5e-4; every other tensor within the 2e-5 / 5e-5 floors or 2 n).  The maximum has no derivative where two cameras tie, and near a
    tie the winner depends on rounding (the fp32 integral images of the reference differ from float64 by ~1e-4 of the map): one flipped
    element moves a whole row of the weight gradient to another camera.  The probe is therefore zero on elements whose two best
    cameras are within 2e-3 max|t| of each other in float64 (ties are pinned by the kernel tests and the duplicated camera)."""
    import vfa_amd
    dev = _dev()
    d = _load(name)
    mods = _mods(d, dev)
    C, L, W = d["ortho"].shape
    probe = torch.randn((C, L, W), generator=torch.Generator().manual_seed(21))
    with torch.no_grad():
        _, _, t64 = _oracle_max(d, torch.float64, grad=True)
    top2 = t64.topk(2, dim=0).values if t64.shape[0] > 1 else torch.cat([t64, torch.full_like(t64, -1e30)])
    clear = (top2[0] - top2[1]) > 2e-3 * float(t64.abs().max())
    print(f"[view max grads] {name}: {float(clear.double().mean()):.1%} of the elements probed")
    assert clear.double().mean() > 0.5
    probe = probe * clear.to(probe.dtype)
    lats = [torch.from_numpy(d[f"lat{s}"]).to(dev).requires_grad_(True) for s in (8, 16, 32)]
    calibs = torch.from_numpy(d["calibs"]).to(dev).requires_grad_(True)
    grid = torch.from_numpy(d["grid"])[None].to(dev).requires_grad_(True)
    out = vfa_amd.aggregate_views(*mods, *lats, calibs, grid, view_reduce="max")
    (out * probe[None].to(dev)).sum().backward()
    refs = {}
    for dt in (torch.float32, torch.float64):
        o, leaves, _ = _oracle_max(d, dt, grad=True)
        (o * probe.to(dt)).sum().backward()
        refs[dt] = {k: v.grad.numpy() for k, v in leaves.items()}
    got = {f"lat{s}": lats[i].grad for i, s in enumerate((8, 16, 32))}
    got.update({f"weight{s}": mods[i].collapse.weight.grad for i, s in enumerate((8, 16, 32))})
    got.update({f"bias{s}": mods[i].collapse.bias.grad for i, s in enumerate((8, 16, 32))})
    got["calibs"], got["grid"] = calibs.grad, grid.grad[0]
    for k, g in got.items():
        g32, g64 = refs[torch.float32][k], refs[torch.float64][k]
        n = _rel(g32, g64)
        hip = g.cpu().numpy().reshape(g64.shape)
        e32, e64 = _rel(hip, g32), _rel(hip, g64)
        floor = 5e-4 if k in ("calibs", "grid") else (5e-5 if k.startswith("lat") else 2e-5)
        lim32, lim64 = max(floor, 2 * n), 1.5 * n + floor
        print(f"[view max grads] {name} d {k}: |hip - fp32| {e32:.2e} (limit {lim32:.2e}), |hip - float64| {e64:.2e} (n {n:.2e})")
        assert e32 <= lim32 and e64 <= lim64, (name, k, e32, lim32, e64, lim64, n)


def test_duplicated_camera_is_that_camera_alone():
    """Camera 1 = a copy of camera 0 (calib and maps): the same forward as camera 0 alone, and the copy's gradient is exactly 0."""
    import vfa_amd
    dev = _dev()
    d = _load("vfanet_mc_nl1.npz")
    mods = _mods(d, dev)
    grid = torch.from_numpy(d["grid"])[None].to(dev)
    one = [torch.from_numpy(d[f"lat{s}"][:1]).to(dev) for s in (8, 16, 32)]
    two = [torch.cat([l, l]).requires_grad_(True) for l in one]
    cal1 = torch.from_numpy(d["calibs"][:1]).to(dev)
    cal2 = torch.cat([cal1, cal1]).requires_grad_(True)
    out2 = vfa_amd.aggregate_views(*mods, *two, cal2, grid, view_reduce="max")
    with torch.no_grad():
        out1 = vfa_amd.aggregate_views(*mods, *[l.clone().requires_grad_(False) for l in one], cal1, grid, view_reduce="max")
    out2.sum().backward()
    for l in two:
        assert l.grad[0].abs().sum() > 0 and not l.grad[1].any()
    assert cal2.grad[0].abs().sum() > 0 and not cal2.grad[1].any()
    # the forward of the training path (bf16 GEMM) and of inference (fp32 MFMA) round differently: compare each with its own kind
    with torch.no_grad():
        two_inf = vfa_amd.aggregate_views(*mods, *[l.detach() for l in two], cal2.detach(), grid, view_reduce="max")
    assert torch.equal(two_inf, out1)
    one_train = [l.clone().requires_grad_(True) for l in one]
    assert torch.equal(out2.detach(), vfa_amd.aggregate_views(*mods, *one_train, cal1, grid, view_reduce="max").detach())


def test_one_camera_equals_project_views_and_the_sum_kernel():
    import vfa_amd
    from vfa_amd import ops
    dev = _dev()
    d = _load("vfanet_mc.npz")
    mods = _mods(d, dev)
    grid = torch.from_numpy(d["grid"])[None].to(dev)
    cal = torch.from_numpy(d["calibs"][1:2]).to(dev)
    lats = [torch.from_numpy(d[f"lat{s}"][1:2]).to(dev) for s in (8, 16, 32)]
    with torch.no_grad():
        out = vfa_amd.aggregate_views(*mods, *lats, cal, grid, view_reduce="max")
        lins = [m.project_views(l, cal, grid) for m, l in zip(mods, lats)]
        want = ops.scale_view_sum(*lins, *(m.collapse.bias for m in mods))
    L, W = grid.shape[1:3]
    assert torch.equal(out, want.view(1, L, W, -1).permute(0, 3, 1, 2))


def test_no_camera_gives_zeros():
    import vfa_amd
    from vfa_amd import ops
    dev = _dev()
    d = _load("vfanet_mc.npz")
    mods = _mods(d, dev)
    grid = torch.from_numpy(d["grid"])[None].to(dev)
    empty = [torch.zeros((0, 256, 4, 4), device=dev) for _ in range(3)]
    out = vfa_amd.aggregate_views(*mods, *empty, torch.zeros((0, 3, 4), device=dev), grid, view_reduce="max")
    assert out.shape == (1, 256) + tuple(grid.shape[1:3]) and not out.any()
    o, a = ops.scale_view_max(*(torch.zeros((0, 5, 8), device=dev),) * 3, None, None, None)
    assert o.shape == (5, 8) and not o.any() and not a.any()


def test_default_is_the_sum_bitwise():
    import vfa_amd
    from vfa_amd.synthetic import make_workload
    dev = _dev()
    wl = make_workload("multiviewc_200x200x1", channels=256, seed=1, n_cam=3)
    grid = wl["grid"][:, 100:164, 0:96].contiguous().to(dev)
    torch.manual_seed(0)
    mods = [vfa_amd.VFA(256, grid_height=wl["grid_height"], cube_size=wl["cube_size"], args=wl["args"]).to(dev) for _ in range(3)]
    lats = [torch.cat([wl["features"][c][s] for c in range(3)]).to(dev) for s in range(3)]
    calibs = wl["calibs"].to(dev)
    with torch.no_grad():
        a = vfa_amd.aggregate_views(*mods, *lats, calibs, grid)
        b = vfa_amd.aggregate_views(*mods, *lats, calibs, grid, view_reduce="sum")
        m = vfa_amd.aggregate_views(*mods, *lats, calibs, grid, view_reduce="max")
    assert torch.equal(a, b)
    assert a.abs().max() > 0 and not torch.equal(a, m)


def test_max_backward_is_bit_reproducible_under_deterministic_mode():
    import vfa_amd
    dev = _dev()
    d = _load("vfanet_mc.npz")
    mods = _mods(d, dev)
    grid = torch.from_numpy(d["grid"])[None].to(dev)
    calibs = torch.from_numpy(d["calibs"]).to(dev)
    probe = torch.randn(d["ortho"].shape, generator=torch.Generator().manual_seed(4)).to(dev)[None]
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        runs = []
        for _ in range(2):
            lats = [torch.from_numpy(d[f"lat{s}"]).to(dev).requires_grad_(True) for s in (8, 16, 32)]
            for m in mods:
                m.zero_grad(set_to_none=True)
            out = vfa_amd.aggregate_views(*mods, *lats, calibs, grid, view_reduce="max")
            (out * probe).sum().backward()
            runs.append([l.grad.clone() for l in lats] + [p.grad.clone() for m in mods for p in m.parameters()])
    finally:
        torch.use_deterministic_algorithms(prev)
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_vfanet_max_forward_backward_and_frames():
    from vfa_amd.synthetic import make_workload
    from vfa_amd.vfanet import VFANet
    dev = _dev()
    wl = make_workload("multiviewc_200x200x1", channels=256, seed=2, n_cam=2)
    torch.manual_seed(0)
    net = VFANet(wl["args"], grid_height=wl["grid_height"], cube_size=wl["cube_size"], view_reduce="max").to(dev)
    grid = wl["grid"][:, 60:84, 40:72].contiguous().to(dev)
    calibs = wl["calibs"].to(dev)
    imgs = torch.rand((2, 2, 3, 128, 192), generator=torch.Generator().manual_seed(1)).to(dev)
    for x in (imgs[0], imgs):  # (N, 3, H, W) and (B, N, 3, H, W)
        net.zero_grad(set_to_none=True)
        out = net(x, calibs, grid)
        assert out["heatmap"].shape[0] == (1 if x.dim() == 4 else 2)
        sum(v.float().sum() for v in out.values()).backward()
        for p in (net.vfa8.collapse.weight, net.vfa32.collapse.bias, net.lat16.weight, net.base.conv1.weight):
            assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0
    net.eval()
    with torch.no_grad():
        batched = net.ortho_features(imgs, calibs, grid)
        frames = torch.cat([net.ortho_features(imgs[b], calibs, grid) for b in range(2)])
        per_cam = [net.ortho_features(imgs[0][c:c + 1], calibs[c:c + 1], grid) for c in range(2)]
    assert batched.shape == (2, 256) + tuple(grid.shape[1:3])
    # (the trunk's convolutions may round differently from call to call: 1e-4 of the largest value, as tests/test_batch_frames.py)
    np.testing.assert_allclose(batched.cpu().numpy(), frames.cpu().numpy(), rtol=1e-4, atol=1e-4 * float(frames.abs().max()))
    # on equal lateral maps the B-frame path is bitwise the per-frame calls
    with torch.no_grad():
        lats = net.laterals(imgs.reshape(4, *imgs.shape[2:]))
        mods = [net.vfa8, net.vfa16, net.vfa32]
        import vfa_amd
        b_out = vfa_amd.aggregate_views(*mods, *lats, calibs, grid, frames=2, view_reduce="max")
        f_out = torch.cat([vfa_amd.aggregate_views(*mods, *(l[2 * b:2 * b + 2] for l in lats), calibs, grid, view_reduce="max")
                           for b in range(2)])
    assert torch.equal(b_out, f_out)
    both = torch.maximum(per_cam[0], per_cam[1]).cpu().numpy()  # (laterals of one image vs two: the trunk's tolerance again)
    np.testing.assert_allclose(frames[:1].cpu().numpy(), both, rtol=1e-4, atol=1e-4 * float(np.abs(both).max()))
    keys = [k for k, _, _ in json.load(open(golden_path("vfanet_state_keys.json")))["resnet18_3D"]]
    assert list(net.state_dict().keys()) == keys


def test_reference_style_loop_agrees():
    """The workaround without the feature: the reference's camera loop through the port's ``VFA.forward`` with torch.maximum."""
    import vfa_amd
    from vfa_amd import lazy
    dev = _dev()
    d = _load("vfanet_mc.npz")
    mods = _mods(d, dev)
    grid = torch.from_numpy(d["grid"])[None].to(dev)
    calibs = torch.from_numpy(d["calibs"]).to(dev)
    lats = [torch.from_numpy(d[f"lat{s}"]).to(dev) for s in (8, 16, 32)]
    with torch.no_grad():
        ortho = None
        for cam in range(calibs.shape[0]):
            f = [lazy.materialize(m(l[cam:cam + 1], calibs[cam], grid)) for m, l in zip(mods, lats)]
            t = (f[0] + f[1]) + f[2]
            ortho = t if ortho is None else torch.maximum(ortho, t)
        got = vfa_amd.aggregate_views(*mods, *lats, calibs, grid, view_reduce="max")
    np.testing.assert_allclose(got.cpu().numpy(), ortho.cpu().numpy(), **_tol(ortho.cpu().numpy()))
