"""Batched inference over B frames of one static rig in ONE pipelined launch (``vfa_pipe_batch_records_f32`` +
``vfa_pipe_batch_collapse_relu_sum_f32``, ``vfa_op.pipe_frames``, ``aggregate_views(..., frames=B)``, ``VFANet`` on (B, N, 3, H, W),
``vfa_bev_nms_batch_f32``) against B single-frame calls and the float64 restatement.   ``-m gpu``.

Every frame of a batch gets lateral maps of its own, at a magnitude of its own (frames 2^-9 ... 2^9 apart), so that a mix-up between
frames -- of images, of outputs, or of the fp16 split's power of two -- shows.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# the tolerance form of tests/test_pipe_frame.py: |err| <= RTOL |want| + ATOL_REL max|want|, per frame
RTOL, ATOL_REL = 1e-4, 1e-5


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _mods(wl, dev, seed=1, scale=3.0, n=3):
    import vfa_amd
    torch.manual_seed(seed)
    mods = [vfa_amd.VFA(256, grid_height=wl["grid_height"], cube_size=wl["cube_size"], args=wl["args"]).to(dev) for _ in range(n)]
    with torch.no_grad():
        for m in mods:  # bigger weights and a negative-leaning bias: the ReLU cuts a real share of the outputs
            m.collapse.weight.mul_(scale)
            m.collapse.bias.uniform_(-0.3, 0.1)
    return mods


def _rig(name, n_cam, crop, origin, dev, seed=3):
    from vfa_amd.synthetic import make_workload
    wl = make_workload(name, channels=256, seed=seed, **({"n_cam": n_cam} if n_cam else {}))
    grid = wl["grid"][:, origin[0]:origin[0] + crop[0], origin[1]:origin[1] + crop[1]].contiguous()
    return wl, grid.to(dev), wl["calibs"].to(dev)


FRAME_SCALES = (1.0, 2.0 ** 9, 2.0 ** -7, 3.0, 2.0 ** -9)


def _frames(wl, B, dev, seed=11):
    """Per scale: (B * n, 256, Hf, Wf), frame-major; frame b = distinct random non-negative maps times FRAME_SCALES[b % 5]."""
    n = wl["n_cam"]
    gen = torch.Generator().manual_seed(seed)
    out = []
    for s in range(3):
        h, w = wl["features"][0][s].shape[-2:]
        maps = torch.relu(torch.randn(B, n, 256, h, w, generator=gen))
        maps *= torch.tensor([FRAME_SCALES[b % len(FRAME_SCALES)] for b in range(B)]).view(B, 1, 1, 1, 1)
        out.append(maps.reshape(B * n, 256, h, w).to(dev))
    return out


def _float64_reference(mods, lats, calibs, grid, wl):
    """sum_scale sum_view relu(vox . W^T + b) in float64 from the bitwise-pinned voxel features of the direct pooling kernel."""
    from vfa_amd import _lib, ops
    dev = grid.device
    n = calibs.shape[0]
    grid_flat = grid.reshape(-1, 3).contiguous()
    want = torch.zeros(grid_flat.shape[0], 256, dtype=torch.float64, device=dev)
    for m, lat in zip(mods, lats):
        zl, co = m._kernel_geometry(dev)
        vox = ops.project_gather(ops.integral_image(lat), calibs.reshape(n, 12).contiguous(), grid_flat, zl, co,
                                 _lib.CONV_KIND[wl["args"].data], wl["args"].image_size[::-1], kernel="direct")
        want += torch.relu(vox.double() @ m.layer_major_weight().double().T + m.collapse.bias.double()).sum(0)
    return want


def _check(name, got, want):
    scale = want.abs().max().item()
    assert scale > 0, name
    torch.testing.assert_close(got.double(), want.double(), rtol=RTOL, atol=ATOL_REL * scale, msg=lambda m: f"{name}: {m}")


def _frame_of(lats, b, n):
    return [l[b * n:(b + 1) * n] for l in lats]


RIGS = [  # workload, cameras, crop, origin
    ("multiviewc_156x156x5", None, (40, 64), (60, 40)),   # cropped shipped MultiviewC: 7 cameras, 5 layers
    ("wildtrack_120x360x8", 7, (24, 96), (50, 130)),      # Wildtrack: 8 layers, many masked boxes
    ("multiviewc_200x200x1", 3, (37, 53), (11, 5)),       # single-layer grid, ragged
]


@pytest.mark.parametrize("name,n_cam,crop,origin", RIGS)
@pytest.mark.parametrize("B", [1, 2, 3, 5])
def test_batched_frames_equal_their_single_frame_calls(name, n_cam, crop, origin, B):
    from vfa_amd import ops, vfa_op
    dev = _dev()
    wl, grid, calibs = _rig(name, n_cam, crop, origin, dev)
    n = calibs.shape[0]
    mods = _mods(wl, dev)
    lats = _frames(wl, B, dev)
    with torch.no_grad(), ops.KernelTimer() as kt:
        got = vfa_op.pipe_frames(mods, lats, calibs, grid, B)
    torch.cuda.synchronize()
    assert kt.summary()["vfa_pipe_batch_collapse_relu_sum_f32"]["launches"] == 1, kt.summary()
    assert tuple(got.shape) == (B, grid.shape[1] * grid.shape[2], 256) and torch.isfinite(got).all()
    with torch.no_grad():
        for b in range(B):
            one = vfa_op.pipe_frame(mods, _frame_of(lats, b, n), calibs, grid)
            _check(f"{name} B={B} frame {b} vs its single-frame call", got[b], one)
            if b < 2 or b == B - 1:
                want = _float64_reference(mods, _frame_of(lats, b, n), calibs, grid, wl)
                _check(f"{name} B={B} frame {b} vs float64", got[b], want)


@pytest.mark.parametrize("terms", [0, 6])
def test_batched_frames_other_arithmetic_and_accumulate(terms):
    from vfa_amd import vfa_op
    dev = _dev()
    wl, grid, calibs = _rig("multiviewc_156x156x5", 4, (24, 40), (60, 40), dev)
    n, B = calibs.shape[0], 3
    mods = _mods(wl, dev)
    lats = _frames(wl, B, dev, seed=5)
    gen = torch.Generator().manual_seed(2)
    base = torch.randn(B, grid.shape[1] * grid.shape[2], 256, generator=gen).to(dev)
    with torch.no_grad():
        got = vfa_op.pipe_frames(mods, lats, calibs, grid, B, terms=terms)
        acc = vfa_op.pipe_frames(mods, lats, calibs, grid, B, terms=terms, out=base.clone(), accumulate=True)
        for b in range(B):
            one = vfa_op.pipe_frame(mods, _frame_of(lats, b, n), calibs, grid, terms=terms)
            _check(f"terms {terms} frame {b}", got[b], one)
            _check(f"terms {terms} accumulate frame {b}", acc[b], base[b].double() + one.double())


def test_batched_frames_in_bands_of_grid_rows(monkeypatch):
    from vfa_amd import ops, vfa_op
    dev = _dev()
    wl, grid, calibs = _rig("multiviewc_156x156x5", 3, (42, 48), (60, 40), dev)
    n, B = calibs.shape[0], 3
    mods = _mods(wl, dev)
    lats = _frames(wl, B, dev, seed=7)
    with torch.no_grad():
        whole = vfa_op.pipe_frames(mods, lats, calibs, grid, B)
        limit = ops.pipe_batch_workspace_bytes(B, n, 16, 48, 5, 3)
        monkeypatch.setattr(vfa_op, "PIPE_WS_LIMIT", limit)  # bands of 12 grid rows
        with ops.KernelTimer() as kt:
            banded = vfa_op.pipe_frames(mods, lats, calibs, grid, B)
        torch.cuda.synchronize()
        assert kt.summary()["vfa_pipe_batch_collapse_relu_sum_f32"]["launches"] >= 2, kt.summary()
        for b in range(B):
            one = vfa_op.pipe_frame(mods, _frame_of(lats, b, n), calibs, grid)
            _check(f"banded frame {b}", banded[b], one)
            _check(f"banded vs whole frame {b}", banded[b], whole[b])


def test_batched_voxel_features_are_bitwise_those_of_single_frame_calls():
    """VFA_FLAG_DUMP_VOX: one view, one scale, one layer -- every frame's pooled rows as the kernel forms them."""
    from vfa_amd import _lib, ops
    dev = _dev()
    wl, grid, calibs = _rig("multiviewc_200x200x1", 2, (40, 48), (150, 0), dev)
    B = 4
    lats = _frames(wl, B, dev, seed=9)
    mods = _mods(wl, dev)
    zl, co = mods[0]._kernel_geometry(dev)
    kind, img_wh = _lib.CONV_KIND[wl["args"].data], wl["args"].image_size[::-1]
    L, W = grid.shape[1:3]
    cam = 0
    lat = lats[0].view(B, 2, *lats[0].shape[1:])[:, cam].contiguous()  # (B, 256, Hf, Wf): camera 0 of every frame
    calib = calibs[cam:cam + 1]
    hw = [tuple(lat.shape[-2:])]
    with torch.no_grad():
        integ = ops.integral_images([lat])
        ws = ops.pipe_batch_records(calib, grid, zl, co, kind, img_wh, hw, B, weights=[mods[0].collapse.weight])
        got = ops.pipe_batch_collapse(integ, [mods[0].collapse.bias], ws, B, (L, W), 1, dump_vox=True)
        for b in range(B):
            one_i = ops.integral_images([lat[b:b + 1]])
            wsp = ops.pipe_records(calib, grid, zl, co, kind, img_wh, hw, weights=[mods[0].collapse.weight])
            one = ops.pipe_collapse(one_i, [mods[0].collapse.bias], wsp, (L, W), 1, dump_vox=True)
            assert one.abs().max() > 0
            assert torch.equal(got[b], one), (b, int((got[b] != one).sum().item()))


def test_two_launches_of_a_batch_are_bitwise_equal():
    from vfa_amd import vfa_op
    dev = _dev()
    wl, grid, calibs = _rig("wildtrack_120x360x8", 5, (24, 64), (50, 130), dev)
    B = 3
    mods = _mods(wl, dev)
    lats = _frames(wl, B, dev, seed=4)
    with torch.no_grad():
        a = vfa_op.pipe_frames(mods, lats, calibs, grid, B).clone()
        b = vfa_op.pipe_frames(mods, lats, calibs, grid, B)
    assert torch.equal(a, b)


def test_a_workspace_made_for_another_batch_is_refused():
    from vfa_amd import _lib, ops
    dev = _dev()
    wl, grid, calibs = _rig("multiviewc_156x156x5", 3, (16, 24), (60, 40), dev)
    mods = _mods(wl, dev)
    lats = _frames(wl, 3, dev, seed=8)
    zl, co = mods[0]._kernel_geometry(dev)
    kind, img_wh = _lib.CONV_KIND[wl["args"].data], wl["args"].image_size[::-1]
    hw = [tuple(l.shape[-2:]) for l in lats]
    L, W = grid.shape[1:3]
    with torch.no_grad():
        ws2 = ops.pipe_batch_records(calibs, grid, zl, co, kind, img_wh, hw, 2, weights=[m.collapse.weight for m in mods])
        integ3 = ops.integral_images(lats)
        sentinel = torch.full((3, L * W, 256), 7.0, device=dev)
        with pytest.raises(_lib.VFAHipError):
            ops.pipe_batch_collapse(integ3, [m.collapse.bias for m in mods], ws2, 3, (L, W), 5, out=sentinel)
        integ1 = ops.integral_images([l[:3] for l in lats])
        one = torch.full((1, L * W, 256), 7.0, device=dev)
        with pytest.raises(_lib.VFAHipError):
            ops.pipe_batch_collapse(integ1, [m.collapse.bias for m in mods], ws2, 1, (L, W), 5, out=one)
        torch.cuda.synchronize()
    assert (sentinel == 7.0).all() and (one == 7.0).all()  # no map was produced
    # ... and the workspace of this batch's own size works
    with torch.no_grad():
        integ2 = ops.integral_images([l[:6] for l in lats])
        got = ops.pipe_batch_collapse(integ2, [m.collapse.bias for m in mods], ws2, 2, (L, W), 5)
    assert torch.isfinite(got).all()


def test_bev_nms_batch_equals_single_frames_and_stays_inside_its_frame():
    from vfa_amd import eval_ops
    dev = _dev()
    gen = torch.Generator().manual_seed(0)
    B, L, W = 4, 37, 53
    heat = (torch.randn(B, 1, L, W, generator=gen) * 3).to(dev)
    got = eval_ops.bev_nms_batch(heat)
    for b in range(B):
        assert torch.equal(got[b:b + 1], eval_ops.bev_nms(heat[b:b + 1])), b
    # a larger peak in the FIRST row of frame 1 must not suppress the peak in the LAST row of frame 0
    h = torch.full((2, 1, L, W), -5.0, device=dev)
    h[0, 0, L - 1, 10] = 1.0
    h[1, 0, 0, 10] = 4.0
    c = eval_ops.bev_nms_batch(h)
    assert c[0, 0, L - 1, 10].item() == pytest.approx(torch.sigmoid(torch.tensor(1.0)).item())
    assert c[1, 0, 0, 10].item() == pytest.approx(torch.sigmoid(torch.tensor(4.0)).item())


def test_aggregate_views_frames_and_frame_geometry_equal_per_frame_calls():
    import vfa_amd
    from vfa_amd import ops, vfa_op
    dev = _dev()
    wl, grid, calibs = _rig("multiviewc_156x156x5", 3, (24, 40), (60, 40), dev)
    n, B = calibs.shape[0], 3
    mods = _mods(wl, dev)
    lats = _frames(wl, B, dev, seed=12)
    L, W = grid.shape[1:3]
    with torch.no_grad():
        with ops.KernelTimer() as kt:
            got = vfa_amd.aggregate_views(*mods, *lats, calibs, grid[None] if grid.dim() == 3 else grid, frames=B)
        torch.cuda.synchronize()
        assert kt.summary()["vfa_pipe_batch_collapse_relu_sum_f32"]["launches"] == 1
        assert tuple(got.shape) == (B, 256, L, W)
        fg = vfa_op.FrameGeometry(mods, calibs, grid, [tuple(l.shape[-2:]) for l in lats])
        stacked = fg.frame(lats)
        assert tuple(stacked.shape) == (B, 256, L, W)
        per_rig = vfa_amd.aggregate_views(*mods, *lats, calibs[None].expand(B, -1, -1, -1), grid, frames=B)  # a rig per frame: the loop
        for b in range(B):
            one = vfa_amd.aggregate_views(*mods, *_frame_of(lats, b, n), calibs, grid)[0]
            _check(f"aggregate_views frames={B}, frame {b}", got[b].permute(1, 2, 0), one.permute(1, 2, 0))
            assert torch.equal(stacked[b], fg.frame(_frame_of(lats, b, n))[0])
            assert torch.equal(per_rig[b], one)


def test_vfanet_on_a_batch_of_frames_equals_stacked_per_frame_forwards():
    import vfa_amd
    from types import SimpleNamespace
    from vfa_amd.vfanet import VFANet
    from vfa_amd.synthetic import ring_cameras
    from vfa_amd.eval_ops import BEVDecoder
    dev = _dev()
    args = SimpleNamespace(data="MultiviewC", image_size=(192, 320))
    torch.manual_seed(0)
    net = VFANet(args, grid_height=96, cube_size=(50, 50, 32), angle_range=36).to(dev).eval()
    B, N = 3, 3
    gen = torch.Generator().manual_seed(4)
    images = (torch.rand(B, N, 3, 192, 320, generator=gen) * torch.tensor([1.0, 0.25, 2.0]).view(B, 1, 1, 1, 1)).to(dev)
    calibs = ring_cameras(N, (600., 500., 0.), 1500., 500., 250., (320, 192)).to(dev)
    grid = vfa_amd.make_grid((1000, 1200), cube_LW=(50, 50), dataset="MultiviewC").to(dev)[None]
    with torch.no_grad():
        out = net(images, calibs, grid)
        singles = [net(images[b], calibs, grid) for b in range(B)]
        ortho = net.ortho_features(images, calibs, grid)
        ortho_1 = [net.ortho_features(images[b], calibs, grid) for b in range(B)]
    # the trunk and the heads are library convolutions, whose algorithm (and so its rounding) may change with the batch size (B * N
    # images into the trunk): 1e-4 of the largest value (measured: <= 4e-5); the batched BEV path itself on equal lateral maps is
    # held to the 1e-4 / 1e-5 form above (test_aggregate_views_frames_and_frame_geometry_equal_per_frame_calls)
    for b in range(B):
        want = ortho_1[b][0]
        torch.testing.assert_close(ortho[b], want, rtol=1e-3, atol=1e-4 * want.abs().max().item(), msg=lambda m: f"BEV map frame {b}: {m}")
    for k, v in out.items():
        assert v.shape[0] == B, k
        for b in range(B):
            want = singles[b][k][0]
            torch.testing.assert_close(v[b], want, rtol=1e-3, atol=1e-4 * want.abs().max().item(), msg=lambda m: f"head {k} frame {b}: {m}")
    dec = BEVDecoder("MultiviewC", (1000, 1200), (50, 50, 32), dimension_mean=[1.0, 2.0, 3.0], topk=20)
    res = dec.decode_frames(out, 0.0)
    assert len(res) == B
    for b in range(B):
        one = dec.batch_decode({k: v[b:b + 1] for k, v in out.items()}, 0.0)
        assert one.keys() == res[b].keys()
        for k in one:
            assert torch.equal(one[k], res[b][k]), (b, k)


def test_batched_aggregate_gradients_are_the_sums_of_the_per_frame_ones():
    import vfa_amd
    dev = _dev()
    wl, grid, calibs = _rig("multiviewc_156x156x5", 2, (16, 24), (60, 40), dev)
    n, B = calibs.shape[0], 3
    mods = _mods(wl, dev)
    lats = [l.requires_grad_() for l in _frames(wl, B, dev, seed=13)]
    gen = torch.Generator().manual_seed(6)
    L, W = grid.shape[1:3]
    R = torch.randn(B, 256, L, W, generator=gen).to(dev)
    params = [p for m in mods for p in (m.collapse.weight, m.collapse.bias)]
    loss = (vfa_amd.aggregate_views(*mods, *lats, calibs, grid, frames=B) * R).sum()
    g_batch = torch.autograd.grad(loss, params + lats)
    g_sum = [torch.zeros_like(p) for p in params]
    g_lat = [torch.zeros_like(l) for l in lats]
    for b in range(B):
        one = [l[b * n:(b + 1) * n] for l in lats]
        lb = (vfa_amd.aggregate_views(*mods, *one, calibs, grid)[0] * R[b]).sum()
        gs = torch.autograd.grad(lb, params + lats)
        g_sum = [a + g for a, g in zip(g_sum, gs[:len(params)])]
        g_lat = [a + g for a, g in zip(g_lat, gs[len(params):])]
    for i, (a, w) in enumerate(zip(g_batch, g_sum + g_lat)):
        assert w.abs().max() > 0, i
        _check(f"gradient {i}", a, w)
