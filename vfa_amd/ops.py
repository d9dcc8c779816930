"""Functional wrappers, one per entry point of ``include/vfa_hip.h`` (no fallback; no autograd but for ``conv3x3_train`` and
``residual_block_train``).

Tensors are device tensors; every call is asynchronous on the current torch HIP stream.
"""
import os
import ctypes

import torch

from . import _lib


def _f32c(t):
    return t.to(dtype=torch.float32).contiguous()


class KernelTimer:
    """Optional per-launch HIP-event timing of the entry points (bench.py's roofline leg).

    Events are recorded on the current torch stream, which is the stream every kernel is launched on.
    ``with KernelTimer() as kt: ...``; after a device synchronise ``kt.summary()`` gives, per entry point,
    the number of launches and their total milliseconds.
    """
    active = None

    def __init__(self, only=None, every=1):
        """``only``: an iterable of entry-point names; other launches are not timed (each timed launch costs two event
        records in the queue, ~3 us apiece on MI355X: 18 per frame slow a 0.9 ms frame by 6 %).  ``every``: time only every
        n-th eligible launch of an entry point (a sample spread over the whole region instead of 1 % of every step)."""
        self.records = []
        self.only = None if only is None else frozenset(only)
        self.every = max(int(every), 1)
        self.seen = {}

    def __enter__(self):
        KernelTimer.active = self
        return self

    def __exit__(self, *exc):
        KernelTimer.active = None

    def summary(self):
        out = {}
        for name, e0, e1, tag in self.records:
            d = out.setdefault(name, dict(launches=0, ms=0.0, by_tag={}))
            ms = e0.elapsed_time(e1)
            d["launches"] += 1
            d["ms"] += ms
            t = d["by_tag"].setdefault(tag, dict(launches=0, ms=0.0))
            t["launches"] += 1
            t["ms"] += ms
        return out


def _launch(name, *args, tag=None):
    kt = KernelTimer.active
    # (the "rows" pre-pass call of the two-stage fused entry point is left untimed: the timed call is the persistent kernel)
    if kt is None or (kt.only is not None and name not in kt.only) or (isinstance(tag, tuple) and tag and tag[-1] == "rows"):
        _lib.call(name, *args)
        return
    if kt.every > 1:
        k = kt.seen.get(name, 0)
        kt.seen[name] = k + 1
        if k % kt.every:
            _lib.call(name, *args)
            return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    _lib.call(name, *args)
    e1.record()
    kt.records.append((name, e0, e1, tag))


def integral_image(features):
    """(n,C,Hf,Wf) -> (n,Hf+2,Wf+2,C) zero-bordered channels-last integral images (reference vfa_op.py:172-173)."""
    _lib.require_device(features)
    features = _f32c(features)
    n, C, Hf, Wf = features.shape
    integral = torch.empty((n, Hf + 2, Wf + 2, C), dtype=torch.float32, device=features.device)
    _launch("vfa_integral_image_f32", _lib.ptr(features), _lib.ptr(integral), n, C, Hf, Wf,
            _lib.current_stream_handle(), tag=(n, C, Hf, Wf))
    return integral


def affine_relu_integral_image(x, scale, shift):
    """Integral images of relu(x * scale[:, :, None, None] + shift[:, :, None, None]) without materialising that map: the
    GroupNorm affine + ReLU of the lateral branch fused into the row scan (reference vfanet.py:72-74 + vfa_op.py:110).
    x (n,C,Hf,Wf), scale / shift (n,C) -> (n,Hf+2,Wf+2,C)."""
    _lib.require_device(x, scale, shift)
    x, scale, shift = _f32c(x), _f32c(scale), _f32c(shift)
    n, C, Hf, Wf = x.shape
    assert tuple(scale.shape) == (n, C) and tuple(shift.shape) == (n, C)
    integral = torch.empty((n, Hf + 2, Wf + 2, C), dtype=torch.float32, device=x.device)
    _launch("vfa_affine_relu_integral_image_f32", _lib.ptr(x), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(integral), n, C, Hf, Wf,
            _lib.current_stream_handle(), tag=(n, C, Hf, Wf))
    return integral


class IntegralImages(list):
    """The integral images of a frame (a plain list of tensors, one per stride) + ``absmax``: per stride the partial maxima of
    |feature| the row scan saw (uint32 bit patterns) -- what the fused frame kernels scale their fp16 operand split by
    (``pool_collapse`` / ``pipe_collapse`` pick it up from here; a plain list works too and costs one extra pass per stride)."""
    absmax = None


def feature_stats_count(n_views, C, Hf):
    return int(_lib.lib().vfa_feature_stats_count(int(n_views), int(C), int(Hf)))


def integral_absmax(integral):
    """Partial maxima of |feature| from a finished integral image (``vfa_integral_absmax_f32``): (n,Hf+2,Wf+2,C) -> int32 tensor."""
    _lib.require_device(integral)
    n, Hp, Wp, C = integral.shape
    out = torch.empty(max(feature_stats_count(n, C, Hp - 2), 1), dtype=torch.int32, device=integral.device)
    _launch("vfa_integral_absmax_f32", _lib.ptr(integral), _lib.ptr(out), n, C, Hp - 2, Wp - 2, _lib.current_stream_handle())
    return out


def _absmax_of(integrals, absmax):
    """The statistics that belong to these integral images: given explicitly, or carried by an ``IntegralImages`` list."""
    if absmax is None:
        absmax = getattr(integrals, "absmax", None)
    if absmax is None:
        return None, None
    absmax = list(absmax)
    assert len(absmax) == len(integrals)
    for i, t in zip(integrals, absmax):
        assert t is None or (t.dtype == torch.int32 and t.is_contiguous()
                             and t.numel() >= feature_stats_count(i.shape[0], i.shape[3], i.shape[1] - 2))
    return absmax, _lib.ptr_array(absmax)


def integral_images(features, scales=None, shifts=None, channels_last=False):
    """The integral images of every feature map of a frame in one launch pair (``vfa_integral_images_f32``): features = one
    (n,C,H_s,W_s) batch per stride -> one (n,H_s+2,W_s+2,C) image per stride, bit-identical to ``integral_image`` of each.
    ``scales`` / ``shifts`` (one (n,C) tensor per map): the fused GroupNorm affine + ReLU of ``affine_relu_integral_image``.
    ``channels_last``: the inputs are (n,H_s,W_s,C) (``lateral_conv``'s output; ``vfa_integral_images_hwc_f32``).
    Returns an ``IntegralImages`` list (the images + the feature statistics of the fp16 operand split)."""
    features = [_f32c(f) for f in features]
    _lib.require_device(*features)
    n = features[0].shape[0]
    C = features[0].shape[3 if channels_last else 1]
    sizes = [tuple(f.shape[1:3]) if channels_last else tuple(f.shape[2:]) for f in features]
    assert all(f.shape[0] == n and f.shape[3 if channels_last else 1] == C for f in features)
    outs = IntegralImages(torch.empty((n, h + 2, w + 2, C), dtype=torch.float32, device=f.device) for f, (h, w) in zip(features, sizes))
    counts = [max(feature_stats_count(n, C, h), 1) for h, _ in sizes]
    stats = torch.empty(sum(counts), dtype=torch.int32, device=features[0].device)  # (every entry is written: no initialisation)
    outs.absmax = list(torch.split(stats, counts))
    affine = scales is not None
    if affine:
        scales, shifts = [_f32c(t) for t in scales], [_f32c(t) for t in shifts]
        assert all(tuple(t.shape) == (n, C) for t in scales + shifts)
    hw = _lib.int_array([v for hw_ in sizes for v in hw_])
    _launch("vfa_integral_images_hwc_f32" if channels_last else "vfa_integral_images_f32", _lib.ptr_array(features),
            _lib.ptr_array(scales) if affine else None, _lib.ptr_array(shifts) if affine else None, _lib.ptr_array(outs),
            _lib.ptr_array(outs.absmax), n, C, len(features), hw, _lib.current_stream_handle(), tag=(n, C, tuple(sizes), affine))
    return outs


_lateral_ws = {}


def lateral_conv(feat, weight, bias, gamma, beta, eps=1e-5):
    """The lateral branch of one scale as far as the integral image needs it (``vfa_lateral_conv_f32``): feat (n,K,h,w) NCHW,
    weight (256,K) or (256,K,1,1), bias / gamma / beta (256) -> y (n,h,w,256) = conv1x1(feat) + bias CHANNELS-LAST, and the
    nn.GroupNorm(16, 256) affine of y as scale, shift (n,256): relu(y * scale + shift) = relu(bn(lat(feat))) (reference
    vfanet.py:72-74).  fp32 FMA chain on the matrix pipe; statistics gathered in the epilogue."""
    _lib.require_device(feat, weight, bias, gamma, beta)
    feat, weight = _f32c(feat), _f32c(weight.reshape(weight.shape[0], -1))
    bias, gamma, beta = _f32c(bias), _f32c(gamma), _f32c(beta)
    n, K, h, w = feat.shape
    assert tuple(weight.shape) == (256, K) and bias.numel() == 256 and gamma.numel() == 256 and beta.numel() == 256
    dev = feat.device
    out = torch.empty((n, h, w, 256), dtype=torch.float32, device=dev)
    scale = torch.empty((n, 256), dtype=torch.float32, device=dev)
    shift = torch.empty((n, 256), dtype=torch.float32, device=dev)
    need = _lib.lib().vfa_lateral_conv_workspace_bytes(n, h, w)
    key = (dev.index, _lib.current_stream(dev).cuda_stream, need)
    ws = _lateral_ws.get(key)  # (one per (device, stream, size): the three scales of a frame are in flight on one stream together)
    if ws is None:
        ws = _lateral_ws[key] = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)
    _launch("vfa_lateral_conv_f32", _lib.ptr(feat), _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(gamma), _lib.ptr(beta), float(eps),
            _lib.ptr(out), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(ws), ws.numel(), n, K, h, w, _lib.current_stream_handle(),
            tag=(n, K, h, w))
    return out, scale, shift


def lateral_convs(branches):
    """``lateral_conv`` for ALL the scales of a frame in three launches (``vfa_lateral_convs_f32``): branches = [(feat, weight, bias,
    gamma, beta, eps), ...] (at most three; the C side orders them by descending K: the deepest map first) -> [(y, scale, shift), ...], bit for bit the per-scale calls
    (reference vfanet.py:72-74 for the three scales).  The small maps' workgroups fill the tail of the large map's launch."""
    if not branches:
        return []
    if len(branches) > 3:
        return [lateral_conv(*b) for b in branches]
    dev = branches[0][0].device
    feats, weights, biases, gammas, betas, epss, outs, scales, shifts, wss, Ks, hws = [], [], [], [], [], [], [], [], [], [], [], []
    n = branches[0][0].shape[0]
    for feat, weight, bias, gamma, beta, eps in branches:
        _lib.require_device(feat, weight, bias, gamma, beta)
        feat, weight = _f32c(feat), _f32c(weight.reshape(weight.shape[0], -1))
        assert feat.shape[0] == n and tuple(weight.shape) == (256, feat.shape[1])
        _, K, h, w = feat.shape
        feats.append(feat), weights.append(weight), biases.append(_f32c(bias)), gammas.append(_f32c(gamma)), betas.append(_f32c(beta))
        epss.append(float(eps)), Ks.append(int(K)), hws.extend((int(h), int(w)))
        outs.append(torch.empty((n, h, w, 256), dtype=torch.float32, device=dev))
        scales.append(torch.empty((n, 256), dtype=torch.float32, device=dev))
        shifts.append(torch.empty((n, 256), dtype=torch.float32, device=dev))
        need = _lib.lib().vfa_lateral_conv_workspace_bytes(n, h, w)
        key = (dev.index, _lib.current_stream(dev).cuda_stream, need, len(wss))  # (one per scale: they are in flight together)
        ws = _lateral_ws.get(key)
        if ws is None:
            ws = _lateral_ws[key] = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)
        wss.append(ws)
    m = len(branches)
    _launch("vfa_lateral_convs_f32", m, _lib.ptr_array(feats), _lib.ptr_array(weights), _lib.ptr_array(biases), _lib.ptr_array(gammas),
            _lib.ptr_array(betas), (ctypes.c_float * m)(*epss), _lib.ptr_array(outs), _lib.ptr_array(scales), _lib.ptr_array(shifts),
            _lib.ptr_array(wss), (ctypes.c_size_t * m)(*[w.numel() for w in wss]), n, _lib.int_array(Ks), _lib.int_array(hws),
            _lib.current_stream_handle(), tag=(n, tuple(Ks), tuple(hws)))
    return list(zip(outs, scales, shifts))


def lateral_convs_train(branches):
    """``lateral_convs`` for training (``vfa_lateral_convs_train_f32``): the same y, scale, shift bit for bit, plus the GroupNorm
    statistics the backward needs -> [(y, scale, shift, mean, rstd), ...] with mean / rstd (n,16) float64 per (view, group)."""
    dev = branches[0][0].device
    n = branches[0][0].shape[0]
    feats, weights, biases, gammas, betas, epss, outs, scales, shifts, means, rstds, wss, Ks, hws = ([] for _ in range(14))
    for feat, weight, bias, gamma, beta, eps in branches:
        _lib.require_device(feat, weight, bias, gamma, beta)
        feat, weight = _f32c(feat), _f32c(weight.reshape(weight.shape[0], -1))
        assert feat.shape[0] == n and tuple(weight.shape) == (256, feat.shape[1])
        _, K, h, w = feat.shape
        feats.append(feat), weights.append(weight), biases.append(_f32c(bias)), gammas.append(_f32c(gamma)), betas.append(_f32c(beta))
        epss.append(float(eps)), Ks.append(int(K)), hws.extend((int(h), int(w)))
        outs.append(torch.empty((n, h, w, 256), dtype=torch.float32, device=dev))
        scales.append(torch.empty((n, 256), dtype=torch.float32, device=dev))
        shifts.append(torch.empty((n, 256), dtype=torch.float32, device=dev))
        means.append(torch.empty((n, 16), dtype=torch.float64, device=dev))
        rstds.append(torch.empty((n, 16), dtype=torch.float64, device=dev))
        need = _lib.lib().vfa_lateral_conv_workspace_bytes(n, h, w)
        key = (dev.index, _lib.current_stream(dev).cuda_stream, need, len(wss))
        ws = _lateral_ws.get(key)
        if ws is None:
            ws = _lateral_ws[key] = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)
        wss.append(ws)
    m = len(branches)
    _launch("vfa_lateral_convs_train_f32", m, _lib.ptr_array(feats), _lib.ptr_array(weights), _lib.ptr_array(biases),
            _lib.ptr_array(gammas), _lib.ptr_array(betas), (ctypes.c_float * m)(*epss), _lib.ptr_array(outs), _lib.ptr_array(scales),
            _lib.ptr_array(shifts), _lib.ptr_array(means), _lib.ptr_array(rstds), _lib.ptr_array(wss),
            (ctypes.c_size_t * m)(*[w.numel() for w in wss]), n, _lib.int_array(Ks), _lib.int_array(hws), _lib.current_stream_handle(),
            tag=(n, tuple(Ks), tuple(hws)))
    return list(zip(outs, scales, shifts, means, rstds))


def lateral_backward_workspace_bytes(n_views, K, h, w):
    """Bytes of the workspace one map's two backward calls share (``vfa_lateral_backward_workspace_bytes``)."""
    return int(_lib.lib().vfa_lateral_backward_workspace_bytes(int(n_views), int(K), int(h), int(w)))


def lateral_scan_backward(grad_integrals, ys, scales, shifts, means, rstds, gammas, Ks, want=(True, True, True)):
    """First half of the producer's backward (``vfa_lateral_scan_backward_f32``), all maps in one launch sequence: d integral
    (n,h+2,w+2,256) per map -> (dzs (n,h,w,256) channels-last, [d bias], [d gamma], [d beta], workspaces).  ``want`` = (bias, gamma,
    beta): the parameter gradients to write (None where not wanted).  The workspaces carry the d y coefficients to
    ``lateral_conv_backward``."""
    m = len(grad_integrals)
    dev = grad_integrals[0].device
    n = grad_integrals[0].shape[0]
    grad_integrals = [_f32c(g) for g in grad_integrals]
    _lib.require_device(*grad_integrals, *ys, *scales, *shifts, *means, *rstds, *gammas)
    hws = [v for g in grad_integrals for v in (g.shape[1] - 2, g.shape[2] - 2)]
    dzs = [torch.empty((n, g.shape[1] - 2, g.shape[2] - 2, 256), dtype=torch.float32, device=dev) for g in grad_integrals]
    wss = [torch.empty(max(lateral_backward_workspace_bytes(n, K, hws[2 * i], hws[2 * i + 1]), 8), dtype=torch.uint8, device=dev)
           for i, K in enumerate(Ks)]
    outs = [[torch.empty(256, dtype=torch.float32, device=dev) if w else None for _ in range(m)] for w in want]
    _launch("vfa_lateral_scan_backward_f32", m, _lib.ptr_array(grad_integrals), _lib.ptr_array(ys), _lib.ptr_array(scales),
            _lib.ptr_array(shifts), _lib.ptr_array(means), _lib.ptr_array(rstds), _lib.ptr_array([_f32c(g) for g in gammas]),
            _lib.ptr_array(dzs), _lib.ptr_array(outs[0]), _lib.ptr_array(outs[1]), _lib.ptr_array(outs[2]), _lib.ptr_array(wss),
            (ctypes.c_size_t * m)(*[w.numel() for w in wss]), n, _lib.int_array(Ks), _lib.int_array(hws), _lib.current_stream_handle(),
            tag=(n, tuple(Ks), tuple(hws), tuple(bool(w) for w in want)))
    return dzs, outs[0], outs[1], outs[2], wss


def lateral_conv_backward(dzs, ys, means, feats, weights, workspaces, want_feat=True, want_weight=True):
    """Second half (``vfa_lateral_conv_backward_f32``): d y formed on the fly, then per map d feat (n,K,h,w) NCHW and d weight
    (256,K), one launch sequence for all maps.  ``want_feat`` / ``want_weight``: a bool or one bool per map; a product that is not
    wanted is not run.  Returns (d feats, d weights), None where not wanted."""
    m = len(dzs)
    n = dzs[0].shape[0]
    dev = dzs[0].device
    feats = [_f32c(f) for f in feats]
    weights = [_f32c(w.reshape(w.shape[0], -1)) for w in weights]
    _lib.require_device(*dzs, *ys, *means, *feats, *weights)
    wf = [bool(want_feat)] * m if isinstance(want_feat, bool) else [bool(w) for w in want_feat]
    ww = [bool(want_weight)] * m if isinstance(want_weight, bool) else [bool(w) for w in want_weight]
    Ks = [int(f.shape[1]) for f in feats]
    hws = [int(v) for f in feats for v in f.shape[2:]]
    g_f = [torch.empty_like(f) if w else None for f, w in zip(feats, wf)]
    g_w = [torch.empty((256, K), dtype=torch.float32, device=dev) if w else None for K, w in zip(Ks, ww)]
    if not (any(wf) or any(ww)):
        return g_f, g_w
    _launch("vfa_lateral_conv_backward_f32", m, _lib.ptr_array(dzs), _lib.ptr_array(ys), _lib.ptr_array(means), _lib.ptr_array(feats),
            _lib.ptr_array(weights), _lib.ptr_array(g_f), _lib.ptr_array(g_w), _lib.ptr_array(workspaces),
            (ctypes.c_size_t * m)(*[w.numel() for w in workspaces]), n, _lib.int_array(Ks), _lib.int_array(hws),
            _lib.current_stream_handle(), tag=(n, tuple(Ks), tuple(hws), tuple(wf), tuple(ww)))
    return g_f, g_w


def _geometry(calibs, grid, z_layers, corner_off, flat=False):
    """The geometry operands as the kernels read them, contiguous fp32 on the device: calibs (n, 12), grid (L, W, 3) -- (cells, 3)
    with ``flat`` --, z_layers (nl), corner_off (8, 3)."""
    _lib.require_device(calibs, grid, z_layers, corner_off)
    grid = grid.reshape(-1, 3) if flat else grid.reshape(grid.shape[-3], grid.shape[-2], 3)
    return _f32c(calibs.reshape(-1, 12)), _f32c(grid), _f32c(z_layers.reshape(-1)), _f32c(corner_off.reshape(8, 3))


def _weight_ptrs(weights, n_scales, shape):
    """Host array of the device pointers of one ``collapse.weight`` of ``shape`` per scale (None -> None)."""
    if weights is None:
        return None
    weights = [_f32c(w) for w in weights]
    assert len(weights) == n_scales and all(tuple(w.shape) == shape for w in weights)
    _lib.require_device(*weights)
    ptrs = _lib.ptr_array(weights)
    ptrs.tensors = weights  # (raw pointers: a converted copy has to live as long as they do)
    return ptrs


def box_params(calibs, grid_flat, z_layers, corner_off, conv_kind, image_wh, feat_hw, crange=(-1, 0.95)):
    """-> box (n,nl,cells,4), area (n,nl,cells), visible (n,nl,cells) uint8 (reference vfa_op.py:64-106)."""
    calibs, grid_flat, z_layers, corner_off = _geometry(calibs, grid_flat, z_layers, corner_off, flat=True)
    n, n_cells, nl = calibs.shape[0], grid_flat.shape[0], z_layers.numel()
    dev = calibs.device
    box = torch.empty((n, nl, n_cells, 4), dtype=torch.float32, device=dev)
    area = torch.empty((n, nl, n_cells), dtype=torch.float32, device=dev)
    visible = torch.empty((n, nl, n_cells), dtype=torch.uint8, device=dev)
    _launch("vfa_box_params_f32", _lib.ptr(calibs), _lib.ptr(grid_flat), _lib.ptr(z_layers), _lib.ptr(corner_off),
              n, n_cells, nl, int(conv_kind), float(image_wh[0]), float(image_wh[1]), int(feat_hw[0]), int(feat_hw[1]),
              float(crange[0]), float(crange[1]), _lib.ptr(box), _lib.ptr(area), _lib.ptr(visible),
              _lib.current_stream_handle())
    return box, area, visible


def gather(integral, box, area, visible, cell_begin=0, cell_count=None, layout=_lib.VOX_LAYER_MAJOR):
    """Box pooling from precomputed box parameters -> vox (n, cell_count, nl*C) (reference vfa_op.py:112-120)."""
    _lib.require_device(integral, box, area, visible)
    n, Hp, Wp, C = integral.shape
    _, nl, n_cells, _ = box.shape
    cell_count = n_cells - cell_begin if cell_count is None else cell_count
    vox = torch.empty((n, cell_count, nl * C), dtype=torch.float32, device=integral.device)
    _launch("vfa_gather_f32", _lib.ptr(integral), _lib.ptr(box), _lib.ptr(area), _lib.ptr(visible), _lib.ptr(vox),
              n, C, Hp - 2, Wp - 2, nl, n_cells, cell_begin, cell_count, layout, _lib.current_stream_handle())
    return vox


GATHER_KERNEL = os.environ.get("VFA_AMD_GATHER", "auto")  # auto | default | direct | tap_cache
_gather_choice = {}


def _pick_gather_kernel(integral, calibs, grid_flat, z_layers, corner_off, conv_kind, image_wh, crange, cell_begin,
                        cell_count):
    """Time the two pooling kernels on this problem (HIP events, one synchronise) and return the faster one's name."""
    n_cells = grid_flat.shape[0]
    count = n_cells - cell_begin if cell_count is None else cell_count
    # the whole problem when its vox fits 1 GiB (every launch of a shape then has one size), else a leading sample of cells
    sample = min(count, max(4096, (1 << 30) // max(1, integral.shape[0] * z_layers.numel() * integral.shape[3] * 4)))
    scratch = torch.empty((integral.shape[0], sample, z_layers.numel() * integral.shape[3]), dtype=torch.float32,
                          device=integral.device)
    best, best_ms = "direct", None
    for name in ("direct", "tap_cache"):
        args = (integral, calibs, grid_flat, z_layers, corner_off, conv_kind, image_wh, crange, cell_begin, sample)
        project_gather(*args, out=scratch, kernel=name)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(2):
            project_gather(*args, out=scratch, kernel=name)
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        if best_ms is None or ms < best_ms:
            best, best_ms = name, ms
    return best


def project_gather(integral, calibs, grid_flat, z_layers, corner_off, conv_kind, image_wh, crange=(-1, 0.95),
                   cell_begin=0, cell_count=None, layout=_lib.VOX_LAYER_MAJOR, out=None, kernel=None):
    """Fused projection + box pooling -> vox (n, cell_count, nl*C) (reference vfa_op.py:64-120).

    ``kernel``: "direct", "tap_cache" (identical results; see include/vfa_hip.h), "default" (the library's static
    rule) or None = ``GATHER_KERNEL`` (env VFA_AMD_GATHER, default "auto": both kernels are timed once per problem shape
    on first use -- which one wins depends on how many taps neighbouring boxes share and how many are masked)."""
    n, Hp, Wp, C = integral.shape
    if kernel is None:
        kernel = GATHER_KERNEL
    if kernel == "auto":
        kernel = "default"
        if C == 256 and (layout & 0xff) == _lib.VOX_LAYER_MAJOR and not torch.cuda.is_current_stream_capturing():
            cells = grid_flat.shape[0] - cell_begin if cell_count is None else cell_count
            key = (integral.device.index, n, Hp, Wp, z_layers.numel(), cells, int(conv_kind), tuple(image_wh), tuple(crange))
            kernel = _gather_choice.get(key)
            if kernel is None:
                kernel = _gather_choice[key] = _pick_gather_kernel(integral, calibs, grid_flat, z_layers, corner_off,
                                                                   conv_kind, image_wh, crange, cell_begin, cell_count)
    if kernel != "default":
        layout = layout | {"direct": _lib.VOX_KERNEL_DIRECT, "tap_cache": _lib.VOX_KERNEL_TAP_CACHE}[kernel]
    _lib.require_device(integral, calibs, grid_flat, z_layers, corner_off)
    n, Hp, Wp, C = integral.shape
    n_cells, nl = grid_flat.shape[0], z_layers.numel()
    cell_count = n_cells - cell_begin if cell_count is None else cell_count
    vox = out if out is not None else torch.empty((n, cell_count, nl * C), dtype=torch.float32,
                                                  device=integral.device)
    _launch("vfa_project_gather_f32", _lib.ptr(integral), _lib.ptr(calibs), _lib.ptr(grid_flat), _lib.ptr(z_layers),
              _lib.ptr(corner_off), _lib.ptr(vox), n, C, Hp - 2, Wp - 2, nl, n_cells, cell_begin, cell_count,
              int(conv_kind), float(image_wh[0]), float(image_wh[1]), float(crange[0]), float(crange[1]), layout,
              _lib.current_stream_handle(), tag=(n, C, Hp - 2, Wp - 2, nl, cell_count))
    return vox


def project_collapse(integral, calibs, grid_flat, z_layers, corner_off, weight_t, conv_kind, image_wh,
                     crange=(-1, 0.95), out=None):
    """Fused projection + box pooling + collapse product -> lin (n, cells, 256), no bias / ReLU (reference
    vfa_op.py:64-123).  ``weight_t`` (nl*C, C_out) = transpose of the layer-major collapse weight.  C = C_out = 256 only."""
    _lib.require_device(integral, calibs, grid_flat, z_layers, corner_off, weight_t)
    n, Hp, Wp, C = integral.shape
    n_cells, nl = grid_flat.shape[0], z_layers.numel()
    c_out = weight_t.shape[1]
    assert weight_t.shape[0] == nl * C and weight_t.is_contiguous()
    lin = out if out is not None else torch.empty((n, n_cells, c_out), dtype=torch.float32, device=integral.device)
    _launch("vfa_project_collapse_f32", _lib.ptr(integral), _lib.ptr(calibs), _lib.ptr(grid_flat), _lib.ptr(z_layers),
            _lib.ptr(corner_off), _lib.ptr(weight_t), _lib.ptr(lin), n, C, Hp - 2, Wp - 2, nl, n_cells, c_out,
            int(conv_kind), float(image_wh[0]), float(image_wh[1]), float(crange[0]), float(crange[1]),
            _lib.current_stream_handle(), tag=(n, C, Hp - 2, Wp - 2, nl, n_cells))
    return lin


def project_gather_ws(integral, calibs, grid_flat, z_layers, corner_off, conv_kind, image_wh, crange=(-1, 0.95),
                      cell_begin=0, cell_count=None, layout=_lib.VOX_LAYER_MAJOR, out=None, workspace=None):
    """Two-kernel form of ``project_gather`` (records through HBM, scalar-loaded by the pooling waves)."""
    _lib.require_device(integral, calibs, grid_flat, z_layers, corner_off)
    n, Hp, Wp, C = integral.shape
    n_cells, nl = grid_flat.shape[0], z_layers.numel()
    cell_count = n_cells - cell_begin if cell_count is None else cell_count
    vox = out if out is not None else torch.empty((n, cell_count, nl * C), dtype=torch.float32,
                                                  device=integral.device)
    need = _lib.lib().vfa_gather_workspace_bytes(n, nl, cell_count)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=integral.device)
    _launch("vfa_project_gather_ws_f32", _lib.ptr(integral), _lib.ptr(calibs), _lib.ptr(grid_flat), _lib.ptr(z_layers),
            _lib.ptr(corner_off), _lib.ptr(vox), _lib.ptr(workspace), workspace.numel(), n, C, Hp - 2, Wp - 2, nl, n_cells,
            cell_begin, cell_count, int(conv_kind), float(image_wh[0]), float(image_wh[1]), float(crange[0]),
            float(crange[1]), layout, _lib.current_stream_handle(), tag=(n, C, Hp - 2, Wp - 2, nl, cell_count))
    return vox


def deterministic_mode(deterministic=None):
    """The ``deterministic`` keyword of the backward wrappers: None = torch's switch (``torch.use_deterministic_algorithms``)."""
    return torch.are_deterministic_algorithms_enabled() if deterministic is None else bool(deterministic)


_det_ws = {}


def det_workspace_bytes(n, nl, cell_count, C, Hf, Wf):
    """Bytes of the workspace of the deterministic scatter (``vfa_gather_backward_det_workspace_bytes``): a function of the shapes."""
    return _lib.lib().vfa_gather_backward_det_workspace_bytes(n, nl, cell_count, C, Hf, Wf)


def project_gather_backward(grad_vox, integral_shape, calibs, grid_flat, z_layers, corner_off, conv_kind, image_wh,
                            crange=(-1, 0.95), cell_begin=0, cell_count=None, out=None, accumulate=False, kernel=None, grid_w=0,
                            deterministic=None, reserved_cus=0):
    """d vox (n, cell_count, nl*C) layer-major -> d integral (n, Hf+2, Wf+2, C) by scatter-add (float atomics).
    ``kernel="direct"`` selects the per-box atomic kernel instead of the LDS-privatised one (C = 256).  ``grid_w``: cells per row of
    the ground grid the cells come from (row-major; 0 = unknown) -- the LDS-privatised scatter then works on patches of 4 x 8 cells
    (``vfa_project_gather_backward_grid_f32``) instead of 32 cells in a line.
    ``deterministic`` (None = torch's switch): the bit-reproducible sort-and-sum scatter (``vfa_project_gather_backward_det_f32``,
    no float atomics; ``kernel`` is ignored, ``reserved_cus`` is passed on and changes nothing) with a workspace cached per
    (device, stream)."""
    _lib.require_device(grad_vox, calibs, grid_flat, z_layers, corner_off, out)
    n, Hp, Wp, C = integral_shape
    n_cells, nl = grid_flat.shape[0], z_layers.numel()
    cell_count = n_cells - cell_begin if cell_count is None else cell_count
    grad_vox = _f32c(grad_vox)
    if out is None:
        out = torch.empty(tuple(integral_shape), dtype=torch.float32, device=grad_vox.device)
        accumulate = False
    grid_w = int(grid_w) if grid_w and n_cells % int(grid_w) == 0 else 0
    if deterministic_mode(deterministic):
        dev = grad_vox.device
        need = det_workspace_bytes(n, nl, cell_count, C, Hp - 2, Wp - 2)
        if need == 0 and n * nl * cell_count > 0:
            raise ValueError(f"deterministic scatter: shapes too large for one call ({n} views x {cell_count} cells x {nl} layers)")
        key = (dev.index, _lib.current_stream(dev).cuda_stream)
        ws = _det_ws.get(key)
        if ws is None or ws.numel() < need:
            ws = _det_ws[key] = None  # (free the old one first)
            ws = _det_ws[key] = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
        _launch("vfa_project_gather_backward_det_f32", _lib.ptr(grad_vox), _lib.ptr(calibs), _lib.ptr(grid_flat),
                _lib.ptr(z_layers), _lib.ptr(corner_off), _lib.ptr(out), n, C, Hp - 2, Wp - 2, nl, n_cells, cell_begin,
                cell_count, grid_w, int(conv_kind), float(image_wh[0]), float(image_wh[1]), float(crange[0]), float(crange[1]),
                (_lib.BWD_ACCUMULATE if accumulate else 0) | _lib.collapse_flags(0, reserved_cus), _lib.ptr(ws), need,
                _lib.current_stream_handle(), tag=(n, C, Hp - 2, Wp - 2, nl, cell_count))
        return out
    _launch("vfa_project_gather_backward_grid_f32", _lib.ptr(grad_vox), _lib.ptr(calibs), _lib.ptr(grid_flat),
            _lib.ptr(z_layers), _lib.ptr(corner_off), _lib.ptr(out), n, C, Hp - 2, Wp - 2, nl, n_cells, cell_begin,
            cell_count, grid_w, int(conv_kind), float(image_wh[0]), float(image_wh[1]), float(crange[0]), float(crange[1]),
            (_lib.BWD_ACCUMULATE if accumulate else 0) | (_lib.VOX_KERNEL_DIRECT if kernel == "direct" else 0),
            _lib.current_stream_handle())
    return out


def project_gather_backward_geometry(grad_vox, integral, calibs, grid_flat, z_layers, corner_off, conv_kind, image_wh,
                                     crange=(-1, 0.95), cell_begin=0, cell_count=None, grad_calibs=None, grad_grid=None, want_calibs=True,
                                     want_grid=True, accumulate=False):
    """d vox (n, cell_count, nl*C) layer-major -> (d calibs (n, 12), d grid (cell_count, 3)) of the box pooling
    (``vfa_project_gather_backward_geometry_f32``: bit-reproducible, no float atomics, whatever torch's deterministic switch says).
    ``integral``: the zero-bordered channels-last images (n, Hf+2, Wf+2, C) the forward pooled from.  ``grad_calibs`` / ``grad_grid``:
    outputs to write (``accumulate``: add, one fp32 add per element -- then every wanted output must be given, ValueError otherwise);
    without ``accumulate`` a missing one is allocated when ``want_*``.  Returns the pair
    (an entry is None when it was neither given nor wanted)."""
    if integral.dim() != 4:
        raise ValueError(f"integral must be (n, Hf+2, Wf+2, C), got {tuple(integral.shape)}")
    n, Hp, Wp, C = integral.shape
    if Hp < 3 or Wp < 3:
        raise ValueError(f"integral must be zero-bordered (n, Hf+2, Wf+2, C), got {tuple(integral.shape)}")
    if tuple(calibs.shape) != (n, 12):
        raise ValueError(f"calibs must be ({n}, 12), got {tuple(calibs.shape)}")
    if grid_flat.dim() != 2 or grid_flat.shape[1] != 3:
        raise ValueError(f"grid_flat must be (n_cells, 3), got {tuple(grid_flat.shape)}")
    n_cells, nl = grid_flat.shape[0], z_layers.numel()
    cell_count = n_cells - cell_begin if cell_count is None else cell_count
    if cell_begin < 0 or cell_count < 0 or cell_begin + cell_count > n_cells:
        raise ValueError(f"cell range [{cell_begin}, {cell_begin + cell_count}) outside the {n_cells} cells")
    if tuple(grad_vox.shape) != (n, cell_count, nl * C):
        raise ValueError(f"grad_vox must be ({n}, {cell_count}, {nl * C}), got {tuple(grad_vox.shape)}")
    for name, t, shape in (("grad_calibs", grad_calibs, (n, 12)), ("grad_grid", grad_grid, (cell_count, 3))):
        if t is not None and (tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous fp32 {shape}, got {tuple(t.shape)} {t.dtype}")
    _lib.require_device(grad_vox, integral, calibs, grid_flat, z_layers, corner_off, grad_calibs, grad_grid)  # (shapes first, then the device)
    dev = grad_vox.device
    if accumulate and ((grad_calibs is None and want_calibs) or (grad_grid is None and want_grid)):
        raise ValueError("accumulate=True adds into the outputs: pass every wanted one (grad_calibs / grad_grid), or want_*=False")
    if grad_calibs is None and want_calibs:
        grad_calibs = torch.empty((n, 12), dtype=torch.float32, device=dev)
    if grad_grid is None and want_grid:
        grad_grid = torch.empty((cell_count, 3), dtype=torch.float32, device=dev)
    if grad_calibs is None and grad_grid is None:
        return None, None
    acc = bool(accumulate)
    grad_vox, integral, calibs, grid_flat = _f32c(grad_vox), _f32c(integral), _f32c(calibs), _f32c(grid_flat)
    need = int(_lib.lib().vfa_gather_backward_geometry_workspace_bytes(n, cell_count)) if grad_calibs is not None else 0
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device=dev) if need else None
    _launch("vfa_project_gather_backward_geometry_f32", _lib.ptr(grad_vox), _lib.ptr(integral), _lib.ptr(calibs),
            _lib.ptr(grid_flat), _lib.ptr(z_layers), _lib.ptr(corner_off), _lib.ptr(grad_calibs), _lib.ptr(grad_grid), n, C, Hp - 2,
            Wp - 2, nl, n_cells, cell_begin, cell_count, int(conv_kind), float(image_wh[0]), float(image_wh[1]), float(crange[0]),
            float(crange[1]), _lib.BWD_ACCUMULATE if acc else 0, _lib.ptr(ws), need, _lib.current_stream_handle(),
            tag=(n, C, Hp - 2, Wp - 2, nl, cell_count))
    return grad_calibs, grad_grid


def integral_image_backward(grad_integral):
    """d integral (n, Hf+2, Wf+2, C) -> d feature (n, C, Hf, Wf).  Destroys ``grad_integral`` (scans it in place)."""
    _lib.require_device(grad_integral)
    grad_integral = _f32c(grad_integral)
    n, Hp, Wp, C = grad_integral.shape
    grad_feature = torch.empty((n, C, Hp - 2, Wp - 2), dtype=torch.float32, device=grad_integral.device)
    _launch("vfa_integral_image_backward_f32", _lib.ptr(grad_integral), _lib.ptr(grad_feature), n, C, Hp - 2, Wp - 2,
            _lib.current_stream_handle())
    return grad_feature


def relu_mask_backward(grad, lin, bias, deterministic=None):
    """-> (grad_lin (n,M,N) = grad * (lin + bias > 0), grad_bias (N) or None).  Backward of both epilogues.
    ``deterministic`` (None = torch's switch): grad_bias from ``column_sum`` (fixed order) instead of the kernel's float atomics."""
    _lib.require_device(grad, lin, bias)
    n, M, N = lin.shape
    grad = _f32c(grad)
    det = deterministic_mode(deterministic)
    if N % 4 != 0 or 1024 % N != 0:  # shapes outside the kernel's fast path: plain torch on the GPU
        pre = lin if bias is None else lin + bias
        g = grad.unsqueeze(0) * (pre > 0)
        if bias is None:
            return g, None
        return g, (column_sum(g.reshape(n * M, N)) if det else g.sum(dim=(0, 1)))
    glin = torch.empty_like(lin)
    gbias = None if (bias is None or det) else torch.empty_like(bias)
    _launch("vfa_relu_mask_backward_f32", _lib.ptr(grad), _lib.ptr(lin), _lib.ptr(bias), _lib.ptr(glin), _lib.ptr(gbias),
            n, M, N, _lib.current_stream_handle())
    if det and bias is not None:
        gbias = column_sum(glin.view(n * M, N))
    return glin, gbias


COLUMN_SUM_WIDTH = 16384  # columns of the first of the two column-sum calls on a tall matrix


def column_sum(x, out=None, accumulate=False):
    """out (N) (+)= column sums of x (rows, N) in a fixed order (``vfa_column_sum_f32``): bit-reproducible, no atomics.  A tall
    matrix is summed in two calls: over the (rows // B, B N) view of its first rows (B = COLUMN_SUM_WIDTH // N; the kernel is
    parallel over columns), then over the (B, N) partial sums followed by the remaining rows.  The order is a function of the shape."""
    _lib.require_device(x, out)
    x = _f32c(x)
    rows, N = x.shape
    if out is None:
        out = torch.empty(N, dtype=torch.float32, device=x.device)
        accumulate = False
    assert tuple(out.shape) == (N,) and out.is_contiguous() and out.dtype == torch.float32
    B = COLUMN_SUM_WIDTH // N if N % 4 == 0 else 1
    if B >= 2 and rows >= 4 * B:
        head = rows // B * B
        part = torch.empty((B + rows - head, N), dtype=torch.float32, device=x.device)
        _launch("vfa_column_sum_f32", _lib.ptr(x), _lib.ptr(part), head // B, B * N, 0, _lib.current_stream_handle(), tag=(rows, N))
        part[B:] = x[head:]
        x, rows = part, part.shape[0]
    _launch("vfa_column_sum_f32", _lib.ptr(x), _lib.ptr(out), rows, N, 1 if accumulate else 0, _lib.current_stream_handle(),
            tag=(rows, N))
    return out


_grad_w_ws = {}


def grad_weight(g_lin, vox, out=None, accumulate=False):
    """out (256, K) (+)= g_lin^T . vox: the weight gradient of ``collapse`` (autograd of nn.Linear's weight, reference vfa_op.py:59, :123
    under trainer.py:41).  g_lin (rows, 256) the masked output gradient, vox (rows, K) the voxel features of the same rows, K a
    multiple of 256.  Six bf16 MFMA products of a three-piece split (sgemm class), fixed summation order (``vfa_grad_weight_f32``)."""
    _lib.require_device(g_lin, vox, out)
    g_lin, vox = _f32c(g_lin), _f32c(vox)
    rows, K = vox.shape
    assert tuple(g_lin.shape) == (rows, 256) and K % 256 == 0
    dev = vox.device
    if out is None:
        out = torch.empty((256, K), dtype=torch.float32, device=dev)
        accumulate = False
    assert tuple(out.shape) == (256, K) and out.is_contiguous() and out.dtype == torch.float32
    need = _lib.lib().vfa_grad_weight_workspace_bytes(rows, K)
    key = (dev.index, _lib.current_stream(dev).cuda_stream)
    ws = _grad_w_ws.get(key)
    if ws is None or ws.numel() < need:
        ws = _grad_w_ws[key] = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)
    _launch("vfa_grad_weight_f32", _lib.ptr(g_lin), _lib.ptr(vox), _lib.ptr(out), rows, K, 1 if accumulate else 0, _lib.ptr(ws),
            ws.numel(), _lib.current_stream_handle(), tag=(rows, K))
    return out


def grad_input(g_lin, w, out=None):
    """out (rows, K) = g_lin (rows, 256) . w (256, K): the gradient of ``collapse``'s input (autograd of nn.Linear's input, reference
    vfa_op.py:123 under trainer.py:41), six bf16 MFMA products of a three-piece split (``vfa_grad_input_f32``)."""
    _lib.require_device(g_lin, w, out)
    g_lin, w = _f32c(g_lin), _f32c(w)
    rows, K = g_lin.shape[0], w.shape[1]
    assert g_lin.shape[1] == 256 and w.shape[0] == 256 and K % 256 == 0
    dev = g_lin.device
    if out is None:
        out = torch.empty((rows, K), dtype=torch.float32, device=dev)
    assert tuple(out.shape) == (rows, K) and out.is_contiguous() and out.dtype == torch.float32
    need = _lib.lib().vfa_grad_input_workspace_bytes(K)
    key = (dev.index, _lib.current_stream(dev).cuda_stream, "x")
    ws = _grad_w_ws.get(key)
    if ws is None or ws.numel() < need:
        ws = _grad_w_ws[key] = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)
    _launch("vfa_grad_input_f32", _lib.ptr(g_lin), _lib.ptr(w), _lib.ptr(out), rows, K, _lib.ptr(ws), ws.numel(),
            _lib.current_stream_handle(), tag=(rows, K))
    return out


def bias_relu_accumulate(lin, bias, out=None, accumulate=False):
    """out (M,N) (+)= sum_v relu(lin[v] + bias) (reference vfa_op.py:124, vfanet.py:82)."""
    _lib.require_device(lin, bias, out)
    n, M, N = lin.shape
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=lin.device)
        accumulate = False
    _launch("vfa_bias_relu_accumulate_f32", _lib.ptr(lin), _lib.ptr(bias), _lib.ptr(out), n, M, N,
              1 if accumulate else 0, _lib.current_stream_handle())
    return out


def scale_view_sum(lin8, lin16, lin32, b8, b16, b32, out=None, accumulate=False):
    """ortho (M,N) (+)= sum_v ((relu(lin8+b8) + relu(lin16+b16)) + relu(lin32+b32)) (reference vfanet.py:79, 82)."""
    _lib.require_device(lin8, lin16, lin32, b8, b16, b32, out)
    n, M, N = lin8.shape
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=lin8.device)
        accumulate = False
    _launch("vfa_scale_view_sum_f32", _lib.ptr(lin8), _lib.ptr(lin16), _lib.ptr(lin32), _lib.ptr(b8), _lib.ptr(b16),
              _lib.ptr(b32), _lib.ptr(out), n, M, N, 1 if accumulate else 0, _lib.current_stream_handle())
    return out


MAX_VIEWS = 256  # the winner index of the max fusion is one byte


def scale_view_max(lin8, lin16, lin32, b8, b16, b32, out=None, want_argmax=True):
    """-> (ortho (M,N) = max_v ((relu(lin8+b8) + relu(lin16+b16)) + relu(lin32+b32)), argmax (M,N) uint8 or None).
    The winner is torch.max(dim=0)'s: the lowest view attaining the maximum, the first NaN view if any (``vfa_scale_view_max_f32``)."""
    _lib.require_device(lin8, lin16, lin32, b8, b16, b32, out)
    n, M, N = lin8.shape
    if tuple(lin16.shape) != (n, M, N) or tuple(lin32.shape) != (n, M, N):
        raise ValueError(f"scale_view_max: lin shapes differ: {tuple(lin8.shape)}, {tuple(lin16.shape)}, {tuple(lin32.shape)}")
    if n > MAX_VIEWS:
        raise ValueError(f"scale_view_max: {n} views, at most {MAX_VIEWS}")
    lin8, lin16, lin32 = _f32c(lin8), _f32c(lin16), _f32c(lin32)
    b8, b16, b32 = (None if b is None else _f32c(b) for b in (b8, b16, b32))
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=lin8.device)
    argmax = torch.empty((M, N), dtype=torch.uint8, device=lin8.device) if want_argmax else None
    _launch("vfa_scale_view_max_f32", _lib.ptr(lin8), _lib.ptr(lin16), _lib.ptr(lin32), _lib.ptr(b8), _lib.ptr(b16), _lib.ptr(b32),
            _lib.ptr(out), _lib.ptr(argmax), n, M, N, _lib.current_stream_handle(), tag=(n, M, N))
    return out, argmax


def scale_view_max_backward(grad, lin8, lin16, lin32, b8, b16, b32, argmax, want_bias=(True, True, True)):
    """Backward of ``scale_view_max``: -> (grad_lin8, grad_lin16, grad_lin32 (n,M,N) dense, grad_b8, grad_b16, grad_b32 (N) or None).
    Each element's gradient goes to its winning view only, through that view's ReLU masks (``vfa_scale_view_max_backward_f32``, no
    float atomics).  The bias gradients are ``column_sum``s of the dense rows (a fixed order): bit-reproducible on every run."""
    _lib.require_device(grad, lin8, lin16, lin32, b8, b16, b32, argmax)
    n, M, N = lin8.shape
    if tuple(argmax.shape) != (M, N) or argmax.dtype != torch.uint8:
        raise ValueError(f"scale_view_max_backward: argmax must be uint8 ({M}, {N}), got {tuple(argmax.shape)} {argmax.dtype}")
    grad, lin8, lin16, lin32, argmax = _f32c(grad), _f32c(lin8), _f32c(lin16), _f32c(lin32), argmax.contiguous()
    b8, b16, b32 = (None if b is None else _f32c(b) for b in (b8, b16, b32))
    glins = [torch.empty((n, M, N), dtype=torch.float32, device=lin8.device) for _ in range(3)]
    _launch("vfa_scale_view_max_backward_f32", _lib.ptr(grad), _lib.ptr(lin8), _lib.ptr(lin16), _lib.ptr(lin32), _lib.ptr(b8),
            _lib.ptr(b16), _lib.ptr(b32), _lib.ptr(argmax), *(_lib.ptr(g) for g in glins), None, None, None, n, M, N,
            _lib.current_stream_handle(), tag=(n, M, N))
    gbias = []
    for g, b, want in zip(glins, (b8, b16, b32), want_bias):
        gbias.append(column_sum(g.view(n * M, N)) if (b is not None and want) else None)
    return (*glins, *gbias)


def collapse_relu_sum(vox, weight, bias, out=None, accumulate=False, terms=0, reserved_cus=0):
    """out (M,N) (+)= sum_v relu(vox[v] @ weight.T + bias) in one bf16-split MFMA kernel (K = N = 256 only; reference
    vfa_op.py:121-124 + vfanet.py:82).  Raises ``VFAHipError`` (VFA_ERR_UNSUPPORTED) for other shapes."""
    _lib.require_device(vox, weight, bias, out)
    vox, weight = _f32c(vox), _f32c(weight)
    bias = None if bias is None else _f32c(bias)
    n, M, K = vox.shape
    N = weight.shape[0]
    assert weight.shape == (N, K), (tuple(weight.shape), K)
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=vox.device)
        accumulate = False
    _launch("vfa_collapse_relu_sum_f32", _lib.ptr(vox), _lib.ptr(weight), _lib.ptr(bias),
            _lib.ptr(out), n, M, K, N, 1 if accumulate else 0, _lib.collapse_flags(terms, reserved_cus),
            _lib.current_stream_handle())
    return out


_gemm_ws = {}


def collapse_gemm(vox2d, weight, out=None, terms=0, reserved_cus=0):
    """lin (M,N) = vox2d (M,K) @ weight (N,K).T as a bf16-split MFMA tile GEMM (N = 256, K a multiple of 128; reference
    vfa_op.py:121-123 without bias).  Raises ``VFAHipError`` (VFA_ERR_UNSUPPORTED) for other shapes."""
    _lib.require_device(vox2d, weight, out)
    vox2d, weight = _f32c(vox2d), _f32c(weight)
    M, K = vox2d.shape
    N = weight.shape[0]
    assert weight.shape == (N, K), (tuple(weight.shape), K)
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=vox2d.device)
    need = _lib.lib().vfa_collapse_gemm_workspace_bytes(K, N)
    key = (vox2d.device.index, _lib.current_stream(vox2d.device).cuda_stream)
    ws = _gemm_ws.get(key)
    if ws is None or ws.numel() < need:  # one scratch buffer per (device, stream): calls on a stream are ordered
        ws = _gemm_ws[key] = torch.empty(max(need, 1), dtype=torch.uint8, device=vox2d.device)
    _launch("vfa_collapse_gemm_f32", _lib.ptr(vox2d), _lib.ptr(weight), _lib.ptr(out), _lib.ptr(ws), ws.numel(), M, K, N,
            _lib.collapse_flags(terms, reserved_cus), _lib.current_stream_handle(), tag=(M, K, N))
    return out


def collapse_gemm_relu_backward(vox, weight, bias, grad_out, terms=0, reserved_cus=0, absmax=None, shift=None, deterministic=None):
    """Training backward behind the fused forward: vox (n, cells, K), weight (256, K) (columns in the order of vox), bias (256) or
    None, grad_out (cells, 256) -> (grad_lin (n, cells, 256) = (vox . W^T + b > 0) ? grad_out : 0, grad_bias (256)) with the ReLU mask
    as the epilogue of the recomputed product (``vfa_collapse_gemm_relu_backward_f32``): the pre-activations never reach memory.
    ``absmax`` (the feature statistics of this scale's integral images, int32) selects the product of the FUSED FRAME KERNELS
    (``vfa_collapse_gemm_relu_backward_f16_f32``: fp16 pieces under the frame's scales); with ``shift`` = this chunk's rows of
    ``sliver_shifts`` ((n or 1, cells) uint8) the mask is then the forward's bit for bit.  ``deterministic`` (None = torch's switch):
    the kernel gets no bias-gradient pointer and grad_bias comes from ``column_sum`` (fixed order) instead of float atomics."""
    _lib.require_device(vox, weight, bias, grad_out)
    det = deterministic_mode(deterministic)
    vox, weight, grad_out = _f32c(vox), _f32c(weight), _f32c(grad_out)
    n, cells, K = vox.shape
    assert tuple(weight.shape) == (256, K) and tuple(grad_out.shape) == (cells, 256)
    bias = None if bias is None else _f32c(bias)
    dev = vox.device
    glin = torch.empty((n, cells, 256), dtype=torch.float32, device=dev)
    gbias = None if det else torch.zeros(256, dtype=torch.float32, device=dev)
    need = _lib.lib().vfa_collapse_gemm_workspace_bytes(K, 256)
    key = (dev.index, _lib.current_stream(dev).cuda_stream)
    ws = _gemm_ws.get(key)
    if ws is None or ws.numel() < need:
        ws = _gemm_ws[key] = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    if absmax is not None:
        _lib.require_device(absmax, shift)
        assert absmax.dtype == torch.int32 and absmax.is_contiguous()
        rows = tiles = None
        if shift is not None:
            assert shift.dtype == torch.uint8 and shift.shape[-1] == cells and shift.numel() in (cells, n * cells)
            rows = shift.reshape(-1, cells).expand(n, cells).contiguous().view(-1)  # one byte per row of the product (view, cell)
            pad = (-rows.numel()) % 128
            tiles = (torch.nn.functional.pad(rows, (0, pad)) if pad else rows).view(-1, 128).amax(dim=1).contiguous()
        _launch("vfa_collapse_gemm_relu_backward_f16_f32", _lib.ptr(vox), _lib.ptr(weight), _lib.ptr(bias) if bias is not None else None,
                _lib.ptr(grad_out), _lib.ptr(glin), _lib.ptr(gbias), _lib.ptr(ws), ws.numel(), n, cells, K, 256, _lib.ptr(absmax),
                absmax.numel(), _lib.ptr(rows) if rows is not None else None, _lib.ptr(tiles) if tiles is not None else None,
                _lib.collapse_flags(0, reserved_cus), _lib.current_stream_handle(), tag=(n, cells, K, "f16"))
    else:
        _launch("vfa_collapse_gemm_relu_backward_f32", _lib.ptr(vox), _lib.ptr(weight), _lib.ptr(bias) if bias is not None else None,
                _lib.ptr(grad_out), _lib.ptr(glin), _lib.ptr(gbias), _lib.ptr(ws), ws.numel(), n, cells, K, 256,
                _lib.collapse_flags(terms, reserved_cus), _lib.current_stream_handle(), tag=(n, cells, K))
    if det:
        gbias = column_sum(glin.view(n * cells, 256))
    return glin, gbias


def sliver_shifts(calibs, grid, z_layers, corner_off, conv_kind, image_wh, feat_hw, per_item, crange=(-1, 0.95)):
    """The sliver shifts of a frame per output row of the collapse product (``vfa_sliver_shifts_u8``): uint8 (n_views, L*W) for the
    serial frame kernel's items (``per_item`` True: single-layer grids, one scale) or (1, L*W) for the pipelined kernel's (tile, scale)
    over all views and layers -- what ``collapse_gemm_relu_backward(..., absmax=..., shift=...)`` needs to repeat the forward's scaling."""
    calibs, grid, z_layers, corner_off = _geometry(calibs, grid, z_layers, corner_off)
    n, (L, W) = calibs.shape[0], grid.shape[:2]
    out = torch.empty((n if per_item else 1, L * W), dtype=torch.uint8, device=calibs.device)
    need = _lib.lib().vfa_sliver_shifts_scratch_bytes(L, W)
    scratch = torch.empty(max(need, 16), dtype=torch.uint8, device=calibs.device)
    _launch("vfa_sliver_shifts_u8", _lib.ptr(calibs), _lib.ptr(grid), _lib.ptr(z_layers), z_layers.numel(), _lib.ptr(corner_off), n, L, W,
            int(conv_kind), float(image_wh[0]), float(image_wh[1]), float(crange[0]), float(crange[1]), int(feat_hw[0]), int(feat_hw[1]),
            1 if per_item else 0, _lib.ptr(out), _lib.ptr(scratch), scratch.numel(), _lib.current_stream_handle(), tag=(n, L, W))
    return out


def frame_records(calibs, grid, z_layers, corner_off, conv_kind, image_wh, feat_hws, weights=None, crange=(-1, 0.95),
                  workspace=None, row_slots=None, cuts=True, terms=0):
    """Geometry of one frame for the fused inference kernel (``pool_collapse``): box records of every (view, cell) for each
    feature scale + the split collapse weights -> workspace tensor (reference vfa_op.py:64-106, set-up of :112-115).

    calibs (n,3,4), grid (L,W,3) or (1,L,W,3), feat_hws = [(Hf,Wf), ...] (1..3 scales), weights = one (256,256) per scale.
    ``cuts=False``: only the boxes (``vfa_frame_boxes_f32``: what the pre-pass of ``pool_collapse`` needs); ``frame_cuts`` then
    adds the work cuts and the weight split."""
    calibs, grid, z_layers, corner_off = _geometry(calibs, grid, z_layers, corner_off)
    n, (L, W) = calibs.shape[0], grid.shape[:2]
    if z_layers.numel() != 1:
        raise _lib.VFAHipError("frame_records / pool_collapse cover single-layer grids (nl = 1) only")
    ns = len(feat_hws)
    need = _lib.lib().vfa_frame_workspace_bytes(n, L, W, ns)
    if row_slots is not None:  # a smaller workspace: fewer pooled-row slots for direct items (the rest takes the second launch)
        lay = frame_workspace_layout(n, L, W, ns)
        need = lay["rows"] + min(int(row_slots), lay["rows_cap"]) * 32 * 256 * 4
        workspace = None
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=calibs.device)
    hw = _lib.int_array([v for f in feat_hws for v in f])
    wts = _weight_ptrs(weights, ns, (256, 256))
    if not cuts:
        _launch("vfa_frame_boxes_f32", _lib.ptr(calibs), _lib.ptr(grid), _lib.ptr(z_layers), _lib.ptr(corner_off), n, L, W,
                int(conv_kind), float(image_wh[0]), float(image_wh[1]), float(crange[0]), float(crange[1]), ns, hw,
                _lib.ptr(workspace), workspace.numel(), _lib.current_stream_handle(), tag=(n, L, W, ns))
        return workspace
    _launch("vfa_frame_records_f32", _lib.ptr(calibs), _lib.ptr(grid), _lib.ptr(z_layers), _lib.ptr(corner_off), n, L, W,
            int(conv_kind), float(image_wh[0]), float(image_wh[1]), float(crange[0]), float(crange[1]), ns, hw, wts, int(terms) & 0xf,
            _lib.ptr(workspace), workspace.numel(), _lib.current_stream_handle(), tag=(n, L, W, ns))
    return workspace


def frame_cuts(workspace, n_views, grid_lw, n_scales, weights=None, terms=0):
    """Second half of ``frame_records(..., cuts=False)``: the work cuts of the persistent kernel + the split collapse weights."""
    _lib.require_device(workspace)
    wts = _weight_ptrs(weights, n_scales, (256, 256))
    _launch("vfa_frame_cuts_f32", int(n_views), int(grid_lw[0]), int(grid_lw[1]), int(n_scales), wts, int(terms) & 0xf, _lib.ptr(workspace),
            workspace.numel(), _lib.current_stream_handle(), tag=(int(n_views), int(grid_lw[0]), int(grid_lw[1]), int(n_scales)))
    return workspace


def pool_collapse(integrals, biases, workspace, grid_lw, out=None, accumulate=False, terms=0, reserved_cus=0, debug=0, stage="all",
                  absmax=None, dump_vox=False):
    """out (L*W, 256) (+)= sum_scale sum_view relu(vox . W^T + b): pooling + collapse + ReLU + view / scale sum in one
    persistent kernel, the voxel features never touch HBM (reference vfa_op.py:112-125, vfanet.py:79, 82).

    integrals = one (n, Hf+2, Wf+2, 256) zero-bordered channels-last integral image per scale (``integral_image``);
    workspace = ``frame_records`` of the same frame.  ``stage``: "all", or the entry point in two calls -- "rows" (the pre-pass
    over the direct items: needs only the boxes of the frame; returns None) and later "main" (everything else)."""
    _lib.require_device(*integrals, workspace, out)
    stage_flag = {"all": 0, "rows": _lib.FLAG_ROWS_ONLY, "main": _lib.FLAG_SKIP_ROWS}[stage]
    ns = len(integrals)
    n = integrals[0].shape[0]
    L, W = grid_lw
    assert all(i.shape[0] == n and i.shape[3] == 256 and i.is_contiguous() and i.dtype == torch.float32 for i in integrals)
    if out is None and stage != "rows":
        out = torch.empty((L * W, 256), dtype=torch.float32, device=integrals[0].device)
        accumulate = False
    # (the kernel gets a raw pointer)
    assert out is None or (out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (L * W, 256)), \
        "out must be a contiguous fp32 (L*W, 256) tensor"
    biases = [None if b is None else _f32c(b) for b in (biases if biases is not None else [None] * ns)]
    hw = _lib.int_array([v for i in integrals for v in (i.shape[1] - 2, i.shape[2] - 2)])
    absmax, absmax_ptrs = _absmax_of(integrals, absmax)
    _launch("vfa_pool_collapse_relu_sum_f32", _lib.ptr_array(list(integrals)), absmax_ptrs, _lib.ptr_array(biases), _lib.ptr(workspace),
            workspace.numel(), _lib.ptr(out) if out is not None else None, n, L, W, ns, hw, 1 if accumulate else 0,
            _lib.collapse_flags(terms, reserved_cus) | ((int(debug) & 0xfff) << 16) | stage_flag | (_lib.FLAG_DUMP_VOX if dump_vox else 0),  # debug: diagnostic build, tools/ only
            _lib.current_stream_handle(), tag=(n, L, W, tuple((i.shape[1] - 2, i.shape[2] - 2) for i in integrals), stage))
    return out


def pool_windows(integral, workspace, grid_lw, n_scales, scale, out=None):
    """Box pooling of one scale from a ``frame_records`` workspace -> vox (n, L*W, 256) fp32, bit-identical to
    ``project_gather`` (reference vfa_op.py:112-120): tap windows through LDS, one quarter of a (view, tile) per workgroup."""
    _lib.require_device(integral, workspace, out)
    n, Hp, Wp, C = integral.shape
    assert C == 256 and integral.is_contiguous() and integral.dtype == torch.float32
    L, W = grid_lw
    vox = out if out is not None else torch.empty((n, L * W, 256), dtype=torch.float32, device=integral.device)
    _launch("vfa_pool_windows_f32", _lib.ptr(integral), _lib.ptr(workspace), workspace.numel(), _lib.ptr(vox), n, L, W,
            int(n_scales), int(scale), Hp - 2, Wp - 2, _lib.current_stream_handle(), tag=(n, C, Hp - 2, Wp - 2, 1, L * W))
    return vox


def frame_workspace_layout(n_views, L, W, n_scales):
    """Offsets inside the ``frame_records`` workspace, for tests and tools: dict with per-scale lists ``live``, ``direct``,
    ``hdrs``, ``recs``, ``wfrag``, ``overflow`` and ``diag``, ``total``, ``counter``, ``rows``, ``rows_cap``, ``tiles_l``,
    ``tiles_w``, ``max_slots``."""
    import ctypes
    off = (ctypes.c_size_t * 25)()
    tiles = (ctypes.c_int * 4)()
    _lib.call("vfa_frame_workspace_layout", int(n_views), int(L), int(W), int(n_scales), off, tiles)
    names = ("live", "direct", "hdrs", "recs", "wfrag")
    out = {nm: [int(off[5 * k + i]) for k in range(n_scales)] for i, nm in enumerate(names)}
    out["overflow"] = [int(off[17 + k]) for k in range(n_scales)]
    out.update(diag=int(off[15]), total=int(off[16]), counter=int(off[20]), rows=int(off[21]), rows_cap=int(off[22]),
               chunks=int(off[23]), ranks=int(off[24]),
               tiles_l=int(tiles[0]), tiles_w=int(tiles[1]), max_slots=int(tiles[2]), n_chunks=int(tiles[3]))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the frame as a producer / consumer pipeline, any number of z-layers (vfa_pipe.hip)
# ---------------------------------------------------------------------------------------------------------------------------------
def pipe_workspace_bytes(n_views, L, W, n_layers, n_scales):
    return int(_lib.lib().vfa_pipe_workspace_bytes(int(n_views), int(L), int(W), int(n_layers), int(n_scales)))


def pipe_records(calibs, grid, z_layers, corner_off, conv_kind, image_wh, feat_hws, weights=None, crange=(-1, 0.95), workspace=None,
                 cuts=True, terms=0):
    """Geometry of one frame for ``pipe_collapse``: box records and tap-window headers of every (view, cell, layer) for each
    feature scale, the work cuts and the split collapse weights -> workspace (reference vfa_op.py:64-106).

    calibs (n,3,4), grid (L,W,3) or (1,L,W,3), z_layers (nl), feat_hws = [(Hf,Wf), ...] (1..3 scales), weights = one
    (256, 256*nl) per scale in the REFERENCE column order c*nl + layer (``collapse.weight`` as it is).  ``cuts=False``: the
    boxes only (``pipe_cuts`` adds the rest).  ``terms``: the product variant ``pipe_collapse`` will be called with (6 = three bf16
    pieces per operand: smaller LDS tap windows, so the geometry has to know)."""
    calibs, grid, z_layers, corner_off = _geometry(calibs, grid, z_layers, corner_off)
    n, (L, W) = calibs.shape[0], grid.shape[:2]
    nl, ns = z_layers.numel(), len(feat_hws)
    need = pipe_workspace_bytes(n, L, W, nl, ns)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=calibs.device)
        # a fresh workspace has no balance state (the geometry calls never touch it: whoever allocates clears it, like
        # `vfa_pipe_balance_f32` mode 0): garbage there could pass for bounds if its tag and signature happened to match
        if need > 0:
            bal = pipe_workspace_layout(n, L, W, nl, ns)["balance"]
            workspace[bal:bal + BALANCE_STATE_BYTES].zero_()
    hw = _lib.int_array([v for f in feat_hws for v in f])
    args = (_lib.ptr(calibs), _lib.ptr(grid), _lib.ptr(z_layers), nl, _lib.ptr(corner_off), n, L, W, int(conv_kind),
            float(image_wh[0]), float(image_wh[1]), float(crange[0]), float(crange[1]), ns, hw)
    if not cuts:
        _launch("vfa_pipe_boxes_f32", *args, int(terms) & 0xf, _lib.ptr(workspace), workspace.numel(), _lib.current_stream_handle(),
                tag=(n, L, W, nl, ns))
        return workspace
    wts = _weight_ptrs(weights, ns, (256, 256 * nl))
    _launch("vfa_pipe_records_f32", *args, wts, int(terms) & 0xf, _lib.ptr(workspace), workspace.numel(), _lib.current_stream_handle(),
            tag=(n, L, W, nl, ns))
    return workspace


def pipe_cuts(workspace, n_views, grid_lw, n_layers, n_scales, weights=None, terms=0):
    """Second half of ``pipe_records(..., cuts=False)``: the work cuts of the persistent kernel + the split collapse weights."""
    _lib.require_device(workspace)
    wts = _weight_ptrs(weights, n_scales, (256, 256 * n_layers))
    _launch("vfa_pipe_cuts_f32", int(n_views), int(grid_lw[0]), int(grid_lw[1]), int(n_layers), int(n_scales), wts, int(terms) & 0xf, _lib.ptr(workspace),
            workspace.numel(), _lib.current_stream_handle(), tag=(int(n_views), int(grid_lw[0]), int(grid_lw[1]), int(n_layers), int(n_scales)))
    return workspace


def pipe_collapse(integrals, biases, workspace, grid_lw, n_layers, out=None, accumulate=False, terms=0, reserved_cus=0, debug=0,
                  absmax=None, dump_vox=False):
    """out (L*W, 256) (+)= sum_scale sum_view relu(vox . W^T + b) for K = n_layers * 256: pooling, collapse, ReLU, view and scale
    sums in one persistent kernel (pooling waves and matrix waves side by side); the voxel features never touch HBM
    (reference vfa_op.py:110-125, vfanet.py:79, 82).  workspace = ``pipe_records`` of the same frame."""
    _lib.require_device(*integrals, workspace, out)
    ns = len(integrals)
    n = integrals[0].shape[0]
    L, W = grid_lw
    assert all(i.shape[0] == n and i.shape[3] == 256 and i.is_contiguous() and i.dtype == torch.float32 for i in integrals)
    if out is None:
        out = torch.empty((L * W, 256), dtype=torch.float32, device=integrals[0].device)
        accumulate = False
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (L * W, 256)
    biases = [None if b is None else _f32c(b) for b in (biases if biases is not None else [None] * ns)]
    hw = _lib.int_array([v for i in integrals for v in (i.shape[1] - 2, i.shape[2] - 2)])
    absmax, absmax_ptrs = _absmax_of(integrals, absmax)
    _launch("vfa_pipe_collapse_relu_sum_f32", _lib.ptr_array(list(integrals)), absmax_ptrs, _lib.ptr_array(biases), _lib.ptr(workspace),
            workspace.numel(), _lib.ptr(out), n, L, W, int(n_layers), ns, hw, 1 if accumulate else 0,
            _lib.collapse_flags(terms, reserved_cus) | ((int(debug) & 0xfff) << 16) | (_lib.FLAG_DUMP_VOX if dump_vox else 0),
            _lib.current_stream_handle(), tag=(n, L, W, int(n_layers), tuple((i.shape[1] - 2, i.shape[2] - 2) for i in integrals)))
    return out


def pipe_balance(workspace, n_views, grid_lw, n_layers, n_scales, reserved_cus=0, reset=False):
    """Balance state of a ``pipe_records`` workspace (``vfa_pipe_balance_f32``).  ``reset``: clear it (once, on a fresh workspace);
    otherwise, from the work cuts ``pipe_records`` has just left there: the bounds of the workgroups' shares that minimise the
    heaviest share -- used by every ``pipe_collapse`` launch of the same size on a frame with the same cuts (static cameras and
    grid); deterministic."""
    _lib.require_device(workspace)
    L, W = grid_lw
    _launch("vfa_pipe_balance_f32", int(n_views), int(L), int(W), int(n_layers), int(n_scales), int(reserved_cus), 0 if reset else 1,
            _lib.ptr(workspace), workspace.numel(), _lib.current_stream_handle())


BALANCE_STATE_BYTES = 8192  # (bounds + launch size + cost signature, and at byte 4096 the workgroups' cycle counts)


def pipe_workspace_layout(n_views, L, W, n_layers, n_scales):
    """Offsets inside the ``pipe_records`` workspace, for tests and tools."""
    import ctypes
    off = (ctypes.c_size_t * 22)()
    tiles = (ctypes.c_int * 5)()
    _lib.call("vfa_pipe_workspace_layout", int(n_views), int(L), int(W), int(n_layers), int(n_scales), off, tiles)
    names = ("live", "hdrs", "recs", "wfrag")
    out = {nm: [int(off[4 * k + i]) for k in range(n_scales)] for i, nm in enumerate(names)}
    out.update(tickets=int(off[12]), globs=int(off[17]), chunks=int(off[13]), ranks=int(off[14]), diag=int(off[15]), total=int(off[16]),
               tiles_l=int(tiles[0]), tiles_w=int(tiles[1]), max_slots=int(tiles[2]), n_chunks=int(tiles[3]),
               max_slots_3piece=int(tiles[4]), balance=int(off[18]), shifts=[int(off[19 + k]) for k in range(n_scales)])
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# batched frames of a static rig: B frames in one pipelined launch (vfa_pipe.hip, vfa_pipe_batch_*)
# ---------------------------------------------------------------------------------------------------------------------------------
def pipe_batch_workspace_bytes(n_frames, n_views, L, W, n_layers, n_scales):
    """Bytes of the workspace of a batch of ``n_frames`` frames -- exactly: the batched calls refuse any other size."""
    return int(_lib.lib().vfa_pipe_batch_workspace_bytes(int(n_frames), int(n_views), int(L), int(W), int(n_layers), int(n_scales)))


def pipe_batch_workspace_layout(n_frames, n_views, L, W, n_layers, n_scales):
    """Offsets inside a batched workspace (``pipe_workspace_layout``'s keys + ``meta``, ``frame_exp``, ``virtual_tiles``)."""
    off = (ctypes.c_size_t * 25)()
    tiles = (ctypes.c_int * 6)()
    _lib.call("vfa_pipe_batch_workspace_layout", int(n_frames), int(n_views), int(L), int(W), int(n_layers), int(n_scales), off, tiles)
    names = ("live", "hdrs", "recs", "wfrag")
    out = {nm: [int(off[4 * k + i]) for k in range(n_scales)] for i, nm in enumerate(names)}
    out.update(tickets=int(off[12]), globs=int(off[17]), chunks=int(off[13]), ranks=int(off[14]), diag=int(off[15]), total=int(off[16]),
               tiles_l=int(tiles[0]), tiles_w=int(tiles[1]), max_slots=int(tiles[2]), n_chunks=int(tiles[3]),
               max_slots_3piece=int(tiles[4]), balance=int(off[18]), shifts=[int(off[19 + k]) for k in range(n_scales)],
               meta=int(off[22]), frame_exp=int(off[23]), virtual_tiles=int(tiles[5]))
    return out


def pipe_batch_records(calibs, grid, z_layers, corner_off, conv_kind, image_wh, feat_hws, n_frames, weights=None, crange=(-1, 0.95),
                       workspace=None, terms=0):
    """``pipe_records`` for a batch of ``n_frames`` frames of one static rig: the geometry once, the work cuts over the frames' virtual
    tiles and the batch record -> a workspace of exactly ``pipe_batch_workspace_bytes`` bytes (allocated when ``workspace`` is None,
    with a cleared balance state)."""
    calibs, grid, z_layers, corner_off = _geometry(calibs, grid, z_layers, corner_off)
    n, (L, W) = calibs.shape[0], grid.shape[:2]
    nl, ns = z_layers.numel(), len(feat_hws)
    need = pipe_batch_workspace_bytes(n_frames, n, L, W, nl, ns)
    if workspace is None:
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=calibs.device)
        if need > 0:
            bal = pipe_batch_workspace_layout(n_frames, n, L, W, nl, ns)["balance"]
            workspace[bal:bal + BALANCE_STATE_BYTES].zero_()
    wts = _weight_ptrs(weights, ns, (256, 256 * nl))
    hw = _lib.int_array([v for f in feat_hws for v in f])
    _launch("vfa_pipe_batch_records_f32", _lib.ptr(calibs), _lib.ptr(grid), _lib.ptr(z_layers), nl, _lib.ptr(corner_off), n, L, W,
            int(conv_kind), float(image_wh[0]), float(image_wh[1]), float(crange[0]), float(crange[1]), ns, hw, wts, int(n_frames),
            int(terms) & 0xf, _lib.ptr(workspace), workspace.numel(), _lib.current_stream_handle(), tag=(int(n_frames), n, L, W, nl, ns))
    return workspace


def pipe_batch_collapse(integrals, biases, workspace, n_frames, grid_lw, n_layers, out=None, accumulate=False, terms=0, reserved_cus=0,
                        debug=0, absmax=None, dump_vox=False):
    """out (B, L*W, 256) (+)= per frame sum_scale sum_view relu(vox . W^T + b), B = ``n_frames`` frames in ONE launch of the pipelined
    kernel.  integrals[k]: (B*n, Hf+2, Wf+2, 256), frame-major; workspace = ``pipe_batch_records`` for the same B."""
    _lib.require_device(*integrals, workspace, out)
    ns, B = len(integrals), int(n_frames)
    L, W = grid_lw
    if B < 1 or integrals[0].shape[0] % B:
        raise ValueError(f"pipe_batch_collapse: {integrals[0].shape[0]} integral images are not {B} frames of equal camera count")
    n = integrals[0].shape[0] // B
    assert all(i.shape[0] == B * n and i.shape[3] == 256 and i.is_contiguous() and i.dtype == torch.float32 for i in integrals)
    if out is None:
        out = torch.empty((B, L * W, 256), dtype=torch.float32, device=integrals[0].device)
        accumulate = False
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (B, L * W, 256)
    biases = [None if b is None else _f32c(b) for b in (biases if biases is not None else [None] * ns)]
    hw = _lib.int_array([v for i in integrals for v in (i.shape[1] - 2, i.shape[2] - 2)])
    absmax, absmax_ptrs = _absmax_of(integrals, absmax)
    _launch("vfa_pipe_batch_collapse_relu_sum_f32", _lib.ptr_array(list(integrals)), absmax_ptrs, _lib.ptr_array(biases),
            _lib.ptr(workspace), workspace.numel(), _lib.ptr(out), B, n, L, W, int(n_layers), ns, hw, 1 if accumulate else 0,
            _lib.collapse_flags(terms, reserved_cus) | ((int(debug) & 0xfff) << 16) | (_lib.FLAG_DUMP_VOX if dump_vox else 0),
            _lib.current_stream_handle(), tag=(B, n, L, W, int(n_layers), tuple((i.shape[1] - 2, i.shape[2] - 2) for i in integrals)))
    return out


def pipe_batch_balance(workspace, n_frames, n_views, grid_lw, n_layers, n_scales, reserved_cus=0, reset=False):
    """``pipe_balance`` for a batched workspace (``vfa_pipe_batch_balance_f32``)."""
    _lib.require_device(workspace)
    L, W = grid_lw
    _launch("vfa_pipe_batch_balance_f32", int(n_frames), int(n_views), int(L), int(W), int(n_layers), int(n_scales), int(reserved_cus),
            0 if reset else 1, _lib.ptr(workspace), workspace.numel(), _lib.current_stream_handle())


def _cells_operands(name, feat, weight, cells):
    _lib.require_device(feat, weight, cells)
    if feat.dtype != torch.float32 or feat.dim() != 4:
        raise ValueError(f"{name}: feat must be float32 (B, C, L, W), got {feat.dtype} {tuple(feat.shape)}")
    B, C, L, W = feat.shape
    if weight.dim() != 4 or tuple(weight.shape[1:]) != (C, 3, 3):
        raise ValueError(f"{name}: weight must be (O, {C}, 3, 3), got {tuple(weight.shape)}")
    if cells.dtype != torch.int32 or cells.dim() != 2 or cells.shape[0] != B:
        raise ValueError(f"{name}: cells must be int32 ({B}, k), got {cells.dtype} {tuple(cells.shape)}")
    return _f32c(weight), cells.contiguous(), (ctypes.c_longlong * 4)(*feat.stride()), (B, C, L, W, weight.shape[0], cells.shape[1])


def conv3x3_at_cells_forward(feat, weight, cells, dilation=1, want_logits=True, want_rotation=False):
    """``F.conv2d(feat, weight, padding=dilation, dilation=dilation)`` at the listed cells only, no autograd
    (``vfa_conv3x3_at_cells_f32``).  feat (B,C,L,W) float32 read through its strides (NCHW or channels-last, never copied), weight
    (O,C,3,3), cells (B,k) int32 flat ``l * W + w`` -> (logits (B,k,O) or None, rotation (B,k) or None).  A cell outside
    ``[0, L * W)`` is a skipped row: zeros.  rotation: the decode's arg-max rule on the logits."""
    weight, cells, stride, (B, C, L, W, O, k) = _cells_operands("conv3x3_at_cells", feat, weight, cells)
    if not (want_logits or want_rotation):
        raise ValueError("conv3x3_at_cells: nothing is asked for")
    dev = feat.device
    logits = torch.empty((B, k, O), dtype=torch.float32, device=dev) if want_logits else None
    rotation = torch.empty((B, k), dtype=torch.float32, device=dev) if want_rotation else None
    ws_bytes = 0 if want_logits else _lib.lib().vfa_conv3x3_at_cells_workspace_bytes(B, k, O)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes else None
    _launch("vfa_conv3x3_at_cells_f32", _lib.ptr(feat), stride, _lib.ptr(weight), _lib.ptr(cells), B, C, L, W, O, k, int(dilation),
            _lib.ptr(logits), _lib.ptr(rotation), _lib.ptr(ws), ws_bytes, _lib.current_stream_handle(), tag=(B, C, L, W, O, k))
    return logits, rotation


def conv3x3_at_cells_backward(grad_logits, feat, weight, cells, dilation=1, want_feat=True, want_weight=True):
    """Backward of ``conv3x3_at_cells_forward``: grad_logits (B,k,O) -> (d_feat (B,C,L,W) contiguous, dense, or None; d_weight
    (O,C,3,3) or None) (``vfa_conv3x3_at_cells_backward_f32``: no float atomics, the same bits on every run)."""
    weight, cells, stride, (B, C, L, W, O, k) = _cells_operands("conv3x3_at_cells_backward", feat, weight, cells)
    _lib.require_device(grad_logits)
    if tuple(grad_logits.shape) != (B, k, O):
        raise ValueError(f"conv3x3_at_cells_backward: grad_logits must be ({B}, {k}, {O}), got {tuple(grad_logits.shape)}")
    grad_logits = _f32c(grad_logits)
    d_feat = torch.empty((B, C, L, W), dtype=torch.float32, device=feat.device) if want_feat else None
    d_weight = torch.empty((O, C, 3, 3), dtype=torch.float32, device=feat.device) if want_weight else None
    if want_feat or want_weight:
        _launch("vfa_conv3x3_at_cells_backward_f32", _lib.ptr(grad_logits), _lib.ptr(feat), stride, _lib.ptr(weight), _lib.ptr(cells),
                B, C, L, W, O, k, int(dilation), _lib.ptr(d_feat), _lib.ptr(d_weight), _lib.current_stream_handle(),
                tag=(B, C, L, W, O, k))
    return d_feat, d_weight


def conv3x3_at_cells(feat, weight, cells, dilation=1, want_rotation=False):
    """A 3x3 convolution (zero padding = dilation, no bias) evaluated only at ``cells (B, k)`` int32 (flat ``l * W + w``; an entry
    outside the map, such as the decode's -1, is a skipped row of zeros) -> ``logits (B, k, O)``, or ``(logits, rotation (B, k))``.
    Differentiable with respect to ``feat`` and ``weight`` (one autograd node on the two entry points, ``vfa_op._ConvAtCells``);
    skipped rows get no gradient, the rotation is not differentiable."""
    from . import vfa_op  # (vfa_op imports this module)
    logits, rotation = vfa_op._ConvAtCells.apply(feat, weight, cells, int(dilation), bool(want_rotation))
    return (logits, rotation) if want_rotation else logits


def _det_f32(name, **tensors):
    """The detection-loss entry points take float32 operands on the device; anything else is refused, not converted."""
    _lib.require_device(*tensors.values())
    for key, t in tensors.items():
        if t is not None and t.dtype != torch.float32:
            raise _lib.VFAHipError(f"{name}: {key} must be float32, got {t.dtype} (unsupported)")


def _strides(t, dims):
    return None if t is None else (ctypes.c_longlong * len(dims))(*[t.stride(d) for d in dims])


def det_targets(location, count, dimension=None, rotation=None, dimension_mean=None, world_size=(1.0, 1.0), grid_lw=(1, 1), kind=0):
    """``vfa_det_targets_f32``: location (B, K, 2|3), count (B) int32 and in 3D dimension (B, K, 3), rotation (B, K) ->
    (cells (B, K) int32, n_pos (B) int32, loc_offset (B, K, 2), dim_offset (B, K, 3) | None, angle_label (B, K) int32 | None).
    One launch, no host wait."""
    _det_f32("det_targets", location=location, dimension=dimension, rotation=rotation)
    _lib.require_device(count)
    if location.dim() != 3 or count.dtype != torch.int32 or count.shape != location.shape[:1]:
        raise ValueError(f"det_targets: location (B, K, 2|3) and count (B) int32, got {tuple(location.shape)}, {count.dtype} {tuple(count.shape)}")
    B, K, width = location.shape
    three_d = dimension is not None or rotation is not None
    if three_d and (dimension is None or rotation is None or dimension_mean is None or tuple(dimension.shape) != (B, K, 3)
                    or tuple(rotation.shape) != (B, K)):
        raise ValueError("det_targets: 3D needs dimension (B, K, 3), rotation (B, K) and dimension_mean (3)")
    dev = location.device
    location, count = location.contiguous(), count.contiguous()
    cells = torch.empty((B, K), dtype=torch.int32, device=dev)
    n_pos = torch.empty((B,), dtype=torch.int32, device=dev)
    loc_offset = torch.empty((B, K, 2), dtype=torch.float32, device=dev)
    dim_offset = torch.empty((B, K, 3), dtype=torch.float32, device=dev) if three_d else None
    label = torch.empty((B, K), dtype=torch.int32, device=dev) if three_d else None
    mean = (ctypes.c_float * 3)(*[float(v) for v in dimension_mean]) if three_d else None
    _launch("vfa_det_targets_f32", _lib.ptr(location), int(width), _lib.ptr(count), _lib.ptr(dimension.contiguous() if three_d else None),
            _lib.ptr(rotation.contiguous() if three_d else None), mean, B, K, int(grid_lw[0]), int(grid_lw[1]), float(world_size[0]),
            float(world_size[1]), int(kind), _lib.ptr(cells), _lib.ptr(n_pos), _lib.ptr(loc_offset), _lib.ptr(dim_offset), _lib.ptr(label),
            _lib.current_stream_handle(), tag=(B, K))
    return cells, n_pos, loc_offset, dim_offset, label


def _det_loss_operands(name, heatmap, gt_heatmap, loc, dim, rot, cells, n_pos, loc_t, dim_t, label, table):
    _det_f32(name, heatmap=heatmap, gt_heatmap=gt_heatmap, loc_offset=loc, dim_offset=dim, rotation_at=rot, loc_target=loc_t,
             dim_target=dim_t, table=table)
    _lib.require_device(cells, n_pos, label)
    if heatmap.dim() != 4 or heatmap.shape[1] != 1:
        raise ValueError(f"{name}: heatmap must be (B, 1, L, W), got {tuple(heatmap.shape)}")
    B, _, L, W = heatmap.shape
    k = cells.shape[1]
    three_d = dim is not None
    R = rot.shape[2] if three_d else 0
    if tuple(gt_heatmap.shape) != (B, L, W) or tuple(loc.shape) != (B, L, W, 2) or tuple(cells.shape) != (B, k) or tuple(n_pos.shape) != (B,):
        raise ValueError(f"{name}: gt_heatmap ({B}, {L}, {W}), loc_offset ({B}, {L}, {W}, 2), cells ({B}, k), n_pos ({B}); got "
                         f"{tuple(gt_heatmap.shape)}, {tuple(loc.shape)}, {tuple(cells.shape)}, {tuple(n_pos.shape)}")
    if cells.dtype != torch.int32 or n_pos.dtype != torch.int32 or tuple(loc_t.shape) != (B, k, 2):
        raise ValueError(f"{name}: cells / n_pos int32 and loc_target ({B}, {k}, 2)")
    if three_d and (rot is None or tuple(dim.shape) != (B, L, W, 3) or tuple(rot.shape) != (B, k, R) or tuple(dim_t.shape) != (B, k, 3)
                    or tuple(label.shape) != (B, k) or label.dtype != torch.int32 or tuple(table.shape) != (R,)):
        raise ValueError(f"{name}: 3D needs dim_offset ({B}, {L}, {W}, 3), rotation_at ({B}, {k}, R), dim_target ({B}, {k}, 3), "
                         f"angle_label ({B}, {k}) int32 and table (R)")
    if any(s < 0 for t in (heatmap, gt_heatmap, loc, dim, rot) if t is not None for s in t.stride()):
        raise _lib.VFAHipError(f"{name}: negative strides are not supported")
    ptrs = [_lib.ptr(heatmap), _strides(heatmap, (0, 2, 3)), _lib.ptr(gt_heatmap), _strides(gt_heatmap, (0, 1, 2)), _lib.ptr(loc),
            _strides(loc, (0, 1, 2, 3)), _lib.ptr(dim), _strides(dim, (0, 1, 2, 3)), _lib.ptr(rot), _strides(rot, (0, 1, 2)),
            _lib.ptr(cells.contiguous()), _lib.ptr(n_pos.contiguous()), _lib.ptr(loc_t.contiguous()),
            _lib.ptr(dim_t.contiguous() if three_d else None), _lib.ptr(label.contiguous() if three_d else None),
            _lib.ptr(table.contiguous() if three_d else None)]
    return ptrs, (B, L, W, k, R)


def det_loss_forward(heatmap, gt_heatmap, loc, dim, rot, cells, n_pos, loc_t, dim_t, label, table, loss_weight=(1.0, 1.0, 1.0, 1.0)):
    """``vfa_det_loss_f32``, no autograd: -> (terms (B, 4) = heat map, location, dimension, angle; loss (B); counts (B, 4) int32).
    Heads are read through their strides (never copied); two launches, no host wait."""
    ptrs, (B, L, W, k, R) = _det_loss_operands("det_loss", heatmap, gt_heatmap, loc, dim, rot, cells, n_pos, loc_t, dim_t, label, table)
    dev = heatmap.device
    terms = torch.zeros((B, 4), dtype=torch.float32, device=dev) if L * W == 0 else torch.empty((B, 4), dtype=torch.float32, device=dev)
    loss = torch.zeros((B,), dtype=torch.float32, device=dev) if L * W == 0 else torch.empty((B,), dtype=torch.float32, device=dev)
    counts = torch.zeros((B, 4), dtype=torch.int32, device=dev) if L * W == 0 else torch.empty((B, 4), dtype=torch.int32, device=dev)
    ws_bytes = _lib.lib().vfa_det_loss_workspace_bytes(B, L, W)
    ws = torch.empty(max(ws_bytes, 4), dtype=torch.uint8, device=dev)
    w = list(loss_weight) + [1.0] * (4 - len(loss_weight))
    _launch("vfa_det_loss_f32", *ptrs, (ctypes.c_float * 4)(*[float(v) for v in w]), B, L, W, k, R, _lib.ptr(ws), ws_bytes,
            _lib.ptr(terms), _lib.ptr(loss), _lib.ptr(counts), _lib.current_stream_handle(), tag=(B, L, W, k, R))
    return terms, loss, counts


def det_loss_backward(coef, counts, heatmap, gt_heatmap, loc, dim, rot, cells, n_pos, loc_t, dim_t, label, table):
    """``vfa_det_loss_backward_f32``: coef (B, 4) = d objective / d terms -> (d_heatmap (B, 1, L, W), d_loc_offset (B, L, W, 2),
    d_dim_offset (B, L, W, 3) | None, d_rotation_at (B, k, R) | None), contiguous, every element written."""
    ptrs, (B, L, W, k, R) = _det_loss_operands("det_loss_backward", heatmap, gt_heatmap, loc, dim, rot, cells, n_pos, loc_t, dim_t, label,
                                                table)
    _det_f32("det_loss_backward", coef=coef)
    _lib.require_device(counts)
    if tuple(coef.shape) != (B, 4) or tuple(counts.shape) != (B, 4) or counts.dtype != torch.int32:
        raise ValueError(f"det_loss_backward: coef ({B}, 4) float32 and counts ({B}, 4) int32")
    dev, three_d = heatmap.device, dim is not None
    make = torch.zeros if L * W == 0 else torch.empty
    d_heat = make((B, 1, L, W), dtype=torch.float32, device=dev)
    d_loc = make((B, L, W, 2), dtype=torch.float32, device=dev)
    d_dim = make((B, L, W, 3), dtype=torch.float32, device=dev) if three_d else None
    d_rot = make((B, k, R), dtype=torch.float32, device=dev) if three_d else None
    _launch("vfa_det_loss_backward_f32", _lib.ptr(coef.contiguous()), *ptrs, _lib.ptr(counts.contiguous()), B, L, W, k, R, _lib.ptr(d_heat),
            _lib.ptr(d_loc), _lib.ptr(d_dim), _lib.ptr(d_rot), _lib.current_stream_handle(), tag=(B, L, W, k, R))
    return d_heat, d_loc, d_dim, d_rot


def _heat_operands(name, location, count):
    _det_f32(name, location=location)
    _lib.require_device(count)
    if location.dim() != 3 or location.shape[2] not in (2, 3) or count.dtype != torch.int32 or count.shape != location.shape[:1]:
        raise ValueError(f"{name}: location (B, K, 2|3) and count (B) int32, got {tuple(location.shape)}, {count.dtype} {tuple(count.shape)}")
    return location.contiguous(), count.contiguous()


def heat_rgk(location, count, dimension, angle_deg, world_size=(1.0, 1.0), grid_lw=(1, 1), kind=0, alpha=0.01, ratio=8):
    """``vfa_heat_rgk_f32``: location (B, K, 2|3), count (B) int32, dimension (B, K, 3) = (h, w, l), angle_deg (B, K) FLOAT64 degrees
    -> (heat (B, L, W) float32, n_clipped (B) int32).  Two memsets and one launch, no host wait."""
    location, count = _heat_operands("heat_rgk", location, count)
    _det_f32("heat_rgk", dimension=dimension)
    _lib.require_device(angle_deg)
    B, K, width = location.shape
    if tuple(dimension.shape) != (B, K, 3) or tuple(angle_deg.shape) != (B, K) or angle_deg.dtype != torch.float64:
        raise ValueError(f"heat_rgk: dimension ({B}, {K}, 3) float32 and angle_deg ({B}, {K}) float64, got {tuple(dimension.shape)}, "
                         f"{angle_deg.dtype} {tuple(angle_deg.shape)}")
    L, W = int(grid_lw[0]), int(grid_lw[1])
    dev = location.device
    make = torch.zeros if B * L * W == 0 else torch.empty
    heat = make((B, L, W), dtype=torch.float32, device=dev)
    n_clipped = make((B,), dtype=torch.int32, device=dev)
    _launch("vfa_heat_rgk_f32", _lib.ptr(location), int(width), _lib.ptr(count), _lib.ptr(dimension.contiguous()),
            _lib.ptr(angle_deg.contiguous()), B, K, L, W, float(world_size[0]), float(world_size[1]), int(kind), float(alpha), int(ratio),
            _lib.ptr(heat), _lib.ptr(n_clipped), _lib.current_stream_handle(), tag=(B, K, L, W))
    return heat, n_clipped


def heat_gk(location, count, table, world_size=(1.0, 1.0), grid_lw=(1, 1), kind=0):
    """``vfa_heat_gk_f32``: location (B, K, 2|3), count (B) int32, table (2r+1, 2r+1) float32 on the device -> heat (B, L, W) float32.
    One memset and two launches, no host wait."""
    location, count = _heat_operands("heat_gk", location, count)
    _det_f32("heat_gk", table=table)
    if table.dim() != 2 or table.shape[0] != table.shape[1] or table.shape[0] % 2 != 1:
        raise ValueError(f"heat_gk: table must be (2r+1, 2r+1), got {tuple(table.shape)}")
    B, K, width = location.shape
    L, W = int(grid_lw[0]), int(grid_lw[1])
    dev = location.device
    heat = (torch.zeros if B * L * W == 0 else torch.empty)((B, L, W), dtype=torch.float32, device=dev)
    ws_bytes = _lib.lib().vfa_heat_workspace_bytes(B, L, W)
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=dev)
    _launch("vfa_heat_gk_f32", _lib.ptr(location), int(width), _lib.ptr(count), _lib.ptr(table.contiguous()), int(table.shape[0] // 2), B, K,
            L, W, float(world_size[0]), float(world_size[1]), int(kind), _lib.ptr(ws), ws_bytes, _lib.ptr(heat),
            _lib.current_stream_handle(), tag=(B, K, L, W))
    return heat


IMAGE_MAX_TAPS, IMAGE_MAX_LENGTH = 17, 16384  # VFA_IMAGE_MAX_TAPS, VFA_IMAGE_MAX_LENGTH
_IMAGE_PLANS = {}     # key -> _ImagePlan, in order of insertion
_IMAGE_PLANS_KEPT = 16


class _ImagePlan:
    """A workspace ``vfa_image_plan`` has filled, the operands it was made from (kept alive: their identity is the key) and the
    streams that are ordered behind the launch that filled it."""

    def __init__(self, workspace, ws_bytes, operands, event, stream_id):
        self.workspace, self.ws_bytes, self.operands, self.event, self.streams = workspace, ws_bytes, operands, event, {stream_id}


def _image_constant(name, value, fill, dev):
    """mean / std -> (what the plan cache compares, a (3) float32 tensor on ``dev``).  Numbers are compared by value.  A tensor is
    compared by identity and version counter -- reading its values would be a host wait --, so an in-place update of a model's
    buffer makes a new plan and a tensor written behind torch's back does not."""
    if value is None:
        value = (fill,) * 3
    if isinstance(value, torch.Tensor):
        if value.numel() != 3:
            raise ValueError(f"image_frontend: {name} needs 3 values, got {tuple(value.shape)}")
        return ("tensor", id(value), value._version), value.detach().to(device=dev, dtype=torch.float32).reshape(3).contiguous()
    values = tuple(float(v) for v in value)
    if len(values) != 3:
        raise ValueError(f"image_frontend: {name} needs 3 values, got {len(values)}")
    return values, None


def image_taps(n_in, n_out):
    """Taps of one axis of the resize (``vfa_resize::ksize_of``)."""
    import math
    return int(math.ceil(max(n_in / n_out, 1.0))) * 2 + 1


def _image_plan(dev, sizes, mean, std):
    """The plan of (device, sizes, mean, std): made on the current stream the first time, then kept.  Another stream waits, on the
    device, for the launch that made it.  Under stream capture nothing is waited for and nothing is kept: a plan made before the
    capture is read (the capture begins behind it), one made inside it belongs to the graph."""
    mean_key, mean_t = _image_constant("mean", mean, 0.0, dev)
    std_key, std_t = _image_constant("std", std, 1.0, dev)
    key = (dev.index if dev.index is not None else _lib.current_device_index(), *sizes, mean_key, std_key)
    stream = _lib.current_stream(dev)
    capturing = torch.cuda.is_current_stream_capturing()
    plan = _IMAGE_PLANS.get(key)
    if plan is None:
        if mean_t is None:
            mean_t = torch.tensor(mean_key, dtype=torch.float32).to(dev, non_blocking=True)
        if std_t is None:
            std_t = torch.tensor(std_key, dtype=torch.float32).to(dev, non_blocking=True)
        ws_bytes = _lib.lib().vfa_image_workspace_bytes(*sizes)
        workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        _launch("vfa_image_plan", *sizes, _lib.ptr(mean_t), _lib.ptr(std_t), _lib.ptr(workspace), ws_bytes, _lib.current_stream_handle(),
                tag=sizes)
        if capturing:
            return _ImagePlan(workspace, ws_bytes, (mean, std, mean_t, std_t), None, stream.cuda_stream)
        event = torch.cuda.Event()
        event.record(stream)
        plan = _IMAGE_PLANS[key] = _ImagePlan(workspace, ws_bytes, (mean, std, mean_t, std_t), event, stream.cuda_stream)
        while len(_IMAGE_PLANS) > _IMAGE_PLANS_KEPT:
            del _IMAGE_PLANS[next(iter(_IMAGE_PLANS))]
    elif stream.cuda_stream not in plan.streams and not capturing:
        stream.wait_event(plan.event)
        plan.workspace.record_stream(stream)
        plan.streams.add(stream.cuda_stream)
    return plan


def image_frontend(frames_u8, size=None, mean=None, std=None, out=None):
    """``vfa_image_frames_u8_f32``: camera frames (N, H, W, 3) or (B, N, H, W, 3) uint8 on the device -> (..., 3, Hout, Wout) float32,
    bit for bit the reference's host chain: Pillow's antialiased bilinear ``transforms.Resize(size)`` (``size = (Hout, Wout)``;
    ``None``: no resize), ``ToTensor`` and ``(x - mean) / std`` (``None``: 0 and 1, plain ``ToTensor``).  A row pitch and an image
    stride are taken as they are (``stride(-1) == 1``, ``stride(-2) == 3``, rows of at least ``3 W`` bytes); other layouts are
    copied.  One launch on the current stream, no host wait; the plan (``vfa_image_plan``: the taps of both axes and the 3 x 256
    table) is made on the first call with these (device, sizes, mean, std) and kept."""
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() not in (4, 5) or frames_u8.shape[-1] != 3:
        raise ValueError(f"image_frontend: frames (N, H, W, 3) or (B, N, H, W, 3) uint8, got {frames_u8.dtype} {tuple(frames_u8.shape)}")
    _lib.require_device(frames_u8, out, *(t for t in (mean, std) if isinstance(t, torch.Tensor)))
    lead, (Hin, Win) = tuple(frames_u8.shape[:-3]), frames_u8.shape[-3:-1]
    Hout, Wout = (Hin, Win) if size is None else (int(size[0]), int(size[1]))
    if min(Hin, Win, Hout, Wout) < 1 or max(Hin, Win, Hout, Wout) > IMAGE_MAX_LENGTH:
        raise ValueError(f"image_frontend: lengths must be in 1 .. {IMAGE_MAX_LENGTH}, got {Hin} x {Win} -> {Hout} x {Wout}")
    if max(image_taps(Hin, Hout), image_taps(Win, Wout)) > IMAGE_MAX_TAPS:
        raise ValueError(f"image_frontend: {Hin} x {Win} -> {Hout} x {Wout} shrinks an axis by more than 8 (more than {IMAGE_MAX_TAPS} taps)")
    flat = frames_u8
    if flat.stride(-1) != 1 or (Win > 1 and flat.stride(-2) != 3) or (Hin > 1 and flat.stride(-3) < 3 * Win):
        flat = flat.contiguous()
    if flat.dim() == 5:
        try:
            flat = flat.view(-1, Hin, Win, 3)       # (one image stride for the B * N images)
        except RuntimeError:
            flat = flat.contiguous().view(-1, Hin, Win, 3)
    N = flat.shape[0]
    dev = frames_u8.device
    if out is None:
        out = torch.empty((*lead, 3, Hout, Wout), dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or tuple(out.shape) != (*lead, 3, Hout, Wout) or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"image_frontend: out must be contiguous float32 {(*lead, 3, Hout, Wout)} on {dev}, got {out.dtype} {tuple(out.shape)}")
    if N == 0:
        return out
    sizes = (int(Hin), int(Win), Hout, Wout)
    plan = _image_plan(dev, sizes, mean, std)
    image_stride = int(flat.stride(0)) if N > 1 else 0                # (the stride of a dimension of one element is anything)
    row_stride = int(flat.stride(1)) if Hin > 1 else 3 * sizes[1]
    _launch("vfa_image_frames_u8_f32", _lib.ptr(flat), image_stride, row_stride, N, sizes[0], sizes[1], _lib.ptr(plan.workspace),
            plan.ws_bytes, _lib.ptr(out), Hout, Wout, _lib.current_stream_handle(), tag=(N, *sizes))
    return out


_CONV_KEPT = {}       # key -> _ConvKept: packed weights and folded BatchNorm vectors, in order of insertion
# A ResNet-34 trunk keeps 35 packs (``trunk_conv``; the stem is not packed) beside the heads' 10 entries, and a model must not re-pack
# per frame.  An entry holds its source parameters too (their identity is the key), so up to this many weights of models no longer in
# use, with their packs, stay on the device until newer entries push them out.
_CONV_KEPT_MAX = 128


class _ConvKept:
    """Device tensors made from parameters by one launch (``vfa_conv3x3_pack_weights_f32``, ``vfa_bn_fold_f32``), the parameters they
    were made from (kept alive: their identity is the key) and the streams ordered behind that launch."""

    def __init__(self, tensors, operands, event, stream_id):
        self.tensors, self.operands, self.event, self.streams = tensors, operands, event, {stream_id}


def _conv_kept(kind, operands, extra, dev, make):
    """``make()`` once per (kind, identity and version counter of every operand, extra), like ``_image_plan``: an in-place update of a
    parameter makes a new entry.  Under stream capture nothing is waited for and nothing is kept."""
    key = (kind, dev.index if dev.index is not None else _lib.current_device_index(), extra,
           *((id(t), t._version) if t is not None else None for t in operands))
    stream = _lib.current_stream(dev)
    capturing = torch.cuda.is_current_stream_capturing()
    kept = _CONV_KEPT.get(key)
    if kept is None:
        tensors = make()
        if capturing:
            return tensors
        event = torch.cuda.Event()
        event.record(stream)
        kept = _CONV_KEPT[key] = _ConvKept(tensors, operands, event, stream.cuda_stream)
        while len(_CONV_KEPT) > _CONV_KEPT_MAX:
            del _CONV_KEPT[next(iter(_CONV_KEPT))]
    elif stream.cuda_stream not in kept.streams and not capturing:
        stream.wait_event(kept.event)
        for t in kept.tensors:
            t.record_stream(stream)
        kept.streams.add(stream.cuda_stream)
    return kept.tensors


def _conv_operands(name, x, weight, *more, kernels=(3,), inference=True):
    """What the dense convolutions share: device float32 operands, inference only (but for ``conv3x3_train``) -> (stride array,
    (B, C, L, W, O))."""
    if inference and torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, weight, *more)):
        raise ValueError(f"{name}: inference only -- an operand requires grad while gradients are enabled (use torch.no_grad())")
    _lib.require_device(x, weight, *more)
    if x.dtype != torch.float32 or x.dim() != 4:
        raise ValueError(f"{name}: x must be float32 (B, C, L, W), got {x.dtype} {tuple(x.shape)}")
    B, C, L, W = x.shape
    if weight.dtype != torch.float32 or weight.dim() != 4 or all(tuple(weight.shape[1:]) != (C, k, k) for k in kernels):
        raise ValueError(f"{name}: weight must be float32 {' or '.join(f'(O, {C}, {k}, {k})' for k in kernels)}, got {weight.dtype} {tuple(weight.shape)}")
    for t in more:
        if t is not None and t.dtype != torch.float32:
            raise ValueError(f"{name}: every operand must be float32, got {t.dtype}")
    return (ctypes.c_longlong * 4)(*x.stride()), (B, C, L, W, weight.shape[0])


def _conv3x3_pack(weight, transposed=False):
    """One launch of ``vfa_conv3x3_pack_weights_f32``, or of ``vfa_conv3x3_pack_weights_transposed_f32`` (the planes of the
    transposed, tap-mirrored weight: the convolution that gives the input gradient) -> (packed, bytes), kept nowhere."""
    O, C = int(weight.shape[0]), int(weight.shape[1])
    nbytes = _lib.lib().vfa_conv3x3_packed_bytes(C, O) if transposed else _lib.lib().vfa_conv3x3_packed_bytes(O, C)
    if nbytes == 0:
        raise ValueError(f"conv3x3: {'O' if transposed else 'C'} must be a multiple of 32, got weight {tuple(weight.shape)}")
    w = weight.detach().contiguous()
    packed = torch.empty(nbytes, dtype=torch.uint8, device=weight.device)
    _launch("vfa_conv3x3_pack_weights_transposed_f32" if transposed else "vfa_conv3x3_pack_weights_f32", _lib.ptr(w), O, C, _lib.ptr(packed),
            nbytes, _lib.current_stream_handle(), tag=(O, C))
    return packed, nbytes


def conv3x3_packed_weight(weight):
    """The pre-split fp16 planes of a (O, C, 3, 3) weight (``vfa_conv3x3_pack_weights_f32``), kept by the weight's identity and version."""
    if _lib.lib().vfa_conv3x3_packed_bytes(int(weight.shape[0]), int(weight.shape[1])) == 0:
        raise ValueError(f"conv3x3: C must be a multiple of 32, got weight {tuple(weight.shape)}")
    packed = _conv_kept("pack", (weight,), None, weight.device, lambda: _conv3x3_pack(weight)[:1])[0]
    return packed, packed.numel()


def bn_fold(bn_weight, bn_bias, running_mean, running_var, eps, bias=None):
    """Eval-mode BatchNorm behind a convolution with ``bias`` as a per-channel epilogue (``vfa_bn_fold_f32``): ``scale = weight /
    sqrt(running_var + eps)``, ``shift = bn_bias + (bias - running_mean) * scale``, made on the device and kept by the identity and
    version of the five tensors."""
    _lib.require_device(running_mean, running_var, bn_weight, bn_bias, bias)
    O, dev = running_mean.numel(), running_mean.device
    operands = (bn_weight, bn_bias, running_mean, running_var, bias)
    for t in operands:
        if t is not None and (t.dtype != torch.float32 or t.numel() != O):
            raise ValueError(f"bn_fold: every operand must be float32 with {O} values, got {t.dtype} {tuple(t.shape)}")

    def make():
        ops_c = [None if t is None else t.detach().contiguous() for t in operands]
        scale, shift = torch.empty(O, dtype=torch.float32, device=dev), torch.empty(O, dtype=torch.float32, device=dev)
        _launch("vfa_bn_fold_f32", *(_lib.ptr(t) for t in ops_c), float(eps), O, _lib.ptr(scale), _lib.ptr(shift),
                _lib.current_stream_handle(), tag=(O,))
        return scale, shift
    return _conv_kept("bn", operands, float(eps), dev, make)


def conv3x3(x, weight, dilation=1, scale=None, shift=None, relu=False):
    """``act(F.conv2d(x, weight, padding=dilation, dilation=dilation) * scale[o] + shift[o])`` at inference on the HIP kernel
    (``vfa_conv3x3_f32``): x (B, C, L, W) float32 read through its strides (NCHW, channels-last or a slice, never copied), C a
    multiple of 32, weight (O, C, 3, 3), dilation 1..4, scale / shift (O) device vectors or None (a bias is ``shift``; eval-mode
    BatchNorm: ``bn_fold``), relu -> (B, O, L, W) contiguous.  The three-product fp16 split of fp32 operands on the matrix pipe,
    per-frame power-of-two scales: the same bits on every run, alone and in a batch; no host wait, capturable.  The pre-split weight
    is kept by the weight's identity and version."""
    stride, (B, C, L, W, O) = _conv_operands("conv3x3", x, weight, scale, shift)
    if not 1 <= int(dilation) <= 4:
        raise ValueError(f"conv3x3: dilation must be 1..4, got {dilation}")
    for name, t in (("scale", scale), ("shift", shift)):
        if t is not None and t.numel() != O:
            raise ValueError(f"conv3x3: {name} must have {O} values, got {tuple(t.shape)}")
    packed, nbytes = conv3x3_packed_weight(weight)
    return _conv3x3_launch(x, stride, packed, nbytes, scale, shift, relu, (B, C, L, W, O), dilation)


def _conv3x3_launch(x, stride, packed, nbytes, scale, shift, relu, sizes, dilation):
    """``vfa_conv3x3_f32`` on checked operands and a packed weight -> (B, O, L, W) contiguous."""
    B, C, L, W, O = sizes
    scale = None if scale is None else scale.detach().contiguous()
    shift = None if shift is None else shift.detach().contiguous()
    out = torch.empty((B, O, L, W), dtype=torch.float32, device=x.device)
    if out.numel() == 0:
        return out
    ws_bytes = _lib.lib().vfa_conv3x3_workspace_bytes(B)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    _launch("vfa_conv3x3_f32", _lib.ptr(x), stride, _lib.ptr(packed), nbytes, _lib.ptr(scale), _lib.ptr(shift), int(bool(relu)), B, C, L, W,
            O, int(dilation), _lib.ptr(out), _lib.ptr(ws), ws_bytes, _lib.current_stream_handle(), tag=(B, C, L, W, O, int(dilation)))
    return out


def conv3x3_input_grad(grad, weight, dilation=1):
    """dL/dx of ``y = F.conv2d(x, weight, padding=dilation, dilation=dilation)`` from grad = dL/dy (B, O, L, W), read through its
    strides: the forward kernel on ``grad`` with the transposed, tap-mirrored weight, packed from ``weight`` (O, C, 3, 3) as it lies
    (``vfa_conv3x3_pack_weights_transposed_f32``) -> (B, C, L, W) contiguous; a frame gives the same bits alone and in a batch."""
    O, C = int(weight.shape[0]), int(weight.shape[1])
    B, _, L, W = grad.shape
    packed, nbytes = _conv3x3_pack(weight, transposed=True)
    return _conv3x3_launch(grad, (ctypes.c_longlong * 4)(*grad.stride()), packed, nbytes, None, None, False, (B, O, L, W, C), dilation)


def conv3x3_weight_grad(grad, x, dilation=1, want_bias=False, want_partials=False):
    """dL/dweight (O, C, 3, 3), and dL/dbias (O) or None, of ``y = F.conv2d(x, weight, bias, padding=dilation, dilation=dilation)``
    from grad = dL/dy (B, O, L, W) and x (B, C, L, W), both read through their strides (``vfa_conv3x3_wgrad_f32``): the three-product
    fp16 split with per-frame power-of-two scales of both operands, slab partials merged in ascending (frame, slab) order in
    float64 -- no float atomics, the same bits on every run.  ``want_partials``: a third result, the float32 partials the merge read,
    (B, slabs, 9, O, C) (a view of the call's workspace; for tests of the merge order)."""
    B, C, L, W = x.shape
    O = int(grad.shape[1])
    dw = torch.empty((O, C, 3, 3), dtype=torch.float32, device=x.device)
    db = torch.empty(O, dtype=torch.float32, device=x.device) if want_bias else None
    ws_bytes = _lib.lib().vfa_conv3x3_wgrad_workspace_bytes(B, O, C, L, W)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=x.device)
    _launch("vfa_conv3x3_wgrad_f32", _lib.ptr(grad), (ctypes.c_longlong * 4)(*grad.stride()), _lib.ptr(x), (ctypes.c_longlong * 4)(*x.stride()),
            B, C, L, W, O, int(dilation), _lib.ptr(dw), _lib.ptr(db), _lib.ptr(ws), ws_bytes, _lib.current_stream_handle(),
            tag=(B, C, L, W, O, int(dilation)))
    if want_partials:
        head = (2 * B * 4 + 255) // 256 * 256   # the two scales of every frame, padded
        return dw, db, ws[head:ws_bytes].view(torch.float32).view(B, -1, 9, O, C)
    return dw, db


class _Conv3x3Train(torch.autograd.Function):
    """``conv3x3_train``: the forward kernel of ``conv3x3``, the input gradient on the same kernel and the weight / bias gradients of
    ``csrc/vfa_conv_grad.hip``.  The packed planes are made per call and kept nowhere: a weight under training changes every step."""

    @staticmethod
    def forward(ctx, x, weight, bias, dilation, stride, sizes):
        packed, nbytes = _conv3x3_pack(weight)
        ctx.save_for_backward(x, weight)
        ctx.dilation, ctx.has_bias = dilation, bias is not None
        return _conv3x3_launch(x, stride, packed, nbytes, None, bias, False, sizes, dilation)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        x, weight = ctx.saved_tensors
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = conv3x3_input_grad(grad, weight, ctx.dilation)
        want_bias = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1] or want_bias:
            dw, db = conv3x3_weight_grad(grad, x, ctx.dilation, want_bias=want_bias)
            dw = dw if ctx.needs_input_grad[1] else None
        return dx, dw, db, None, None, None


def conv3x3_train(x, weight, bias=None, dilation=1):
    """``F.conv2d(x, weight, bias, padding=dilation, dilation=dilation)`` with gradients, on the HIP kernels: x (B, C, L, W) float32
    read through its strides, weight (O, C, 3, 3), C and O multiples of 32, bias (O) or None, dilation 1..4 -> (B, O, L, W)
    contiguous, the same bits as ``conv3x3(x.detach(), weight.detach(), dilation, shift=bias)``.  Backward (once differentiable):
    ``conv3x3_input_grad`` and ``conv3x3_weight_grad`` for the operands that require a gradient -- fixed summation order, no float
    atomics, the same bits on every run without ``torch.use_deterministic_algorithms``; no host wait, capturable."""
    stride, sizes = _conv_operands("conv3x3_train", x, weight, bias, inference=False)
    B, C, L, W, O = sizes
    if C % 32 or O % 32:
        raise ValueError(f"conv3x3_train: C and O must be multiples of 32, got weight {tuple(weight.shape)}")
    if not 1 <= int(dilation) <= 4:
        raise ValueError(f"conv3x3_train: dilation must be 1..4, got {dilation}")
    if bias is not None and bias.numel() != O:
        raise ValueError(f"conv3x3_train: bias must have {O} values, got {tuple(bias.shape)}")
    return _Conv3x3Train.apply(x, weight, bias, int(dilation), stride, sizes)


def conv3x3_few(x, weight, dilation=1, affine=None):
    """``F.conv2d(x', weight, padding=dilation, dilation=dilation)`` for 1..4 outputs without bias, in fp32 ``fmaf``
    (``vfa_conv3x3_few_f32``).  ``affine = (a, b)``, both (B, C): ``x' = relu(a[b, c] * x + b[b, c])`` applied as the taps are read
    (``group_norm_affine``: GroupNorm and ReLU without writing the normalised map; the zero padding is applied to ``x'``);
    ``None``: ``x' = x``.  x is read through its strides -> (B, O, L, W) contiguous."""
    a, b = (None, None) if affine is None else affine
    stride, (B, C, L, W, O) = _conv_operands("conv3x3_few", x, weight, a, b)
    if not 1 <= O <= 4 or not 1 <= int(dilation) <= 4 or C % 4:
        raise ValueError(f"conv3x3_few: 1..4 outputs, dilation 1..4 and C a multiple of 4, got weight {tuple(weight.shape)}, dilation {dilation}")
    if affine is not None:
        if tuple(a.shape) != (B, C) or tuple(b.shape) != (B, C):
            raise ValueError(f"conv3x3_few: affine must be two ({B}, {C}) tensors, got {tuple(a.shape)} and {tuple(b.shape)}")
        a, b = a.contiguous(), b.contiguous()
    w = weight.detach().contiguous()
    out = torch.empty((B, O, L, W), dtype=torch.float32, device=x.device)
    if out.numel():
        _launch("vfa_conv3x3_few_f32", _lib.ptr(x), stride, _lib.ptr(w), _lib.ptr(a), _lib.ptr(b), B, C, L, W, O, int(dilation),
                _lib.ptr(out), _lib.current_stream_handle(), tag=(B, C, L, W, O, int(dilation)))
    return out


def group_norm_affine(x, groups, weight, bias, eps):
    """GroupNorm of x (B, C, L, W) as a per (frame, channel) affine (``vfa_group_norm_affine_f32``): ``F.group_norm(x, groups, weight,
    bias, eps) == a[b, c] * x + b[b, c]`` with the statistics of each (frame, group) summed in float64 in a fixed order ->
    (a, b), both (B, C) float32: the prologue of ``conv3x3_few``."""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, weight, bias)):
        raise ValueError("group_norm_affine: inference only -- an operand requires grad while gradients are enabled (use torch.no_grad())")
    _lib.require_device(x, weight, bias)
    if x.dtype != torch.float32 or x.dim() != 4 or int(groups) < 1 or x.shape[1] % int(groups):
        raise ValueError(f"group_norm_affine: x must be float32 (B, C, L, W) with groups | C, got {x.dtype} {tuple(x.shape)}, groups {groups}")
    B, C, L, W = x.shape
    for t in (weight, bias):
        if t is not None and (t.dtype != torch.float32 or t.numel() != C):
            raise ValueError(f"group_norm_affine: weight / bias must be float32 ({C}), got {t.dtype} {tuple(t.shape)}")
    weight = None if weight is None else weight.detach().contiguous()
    bias = None if bias is None else bias.detach().contiguous()
    a, b = torch.empty((B, C), dtype=torch.float32, device=x.device), torch.empty((B, C), dtype=torch.float32, device=x.device)
    if x.numel() == 0:
        raise ValueError("group_norm_affine: an empty map has no statistics")
    ws_bytes = _lib.lib().vfa_group_norm_workspace_bytes(B, int(groups))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    _launch("vfa_group_norm_affine_f32", _lib.ptr(x), (ctypes.c_longlong * 4)(*x.stride()), _lib.ptr(weight), _lib.ptr(bias), float(eps), B, C,
            L, W, int(groups), _lib.ptr(a), _lib.ptr(b), _lib.ptr(ws), ws_bytes, _lib.current_stream_handle(), tag=(B, C, L, W, int(groups)))
    return a, b


def trunk_packed_weight(weight):
    """The pre-split fp16 planes of a (O, C, 3, 3) or (O, C, 1, 1) weight (``vfa_trunk_pack_weights_f32``), kept by the weight's
    identity and version like ``conv3x3_packed_weight`` (the same table: ``_CONV_KEPT_MAX`` holds a ResNet-34 trunk and the heads)."""
    O, C, taps = int(weight.shape[0]), int(weight.shape[1]), int(weight.shape[2]) * int(weight.shape[3])
    nbytes = _lib.lib().vfa_trunk_packed_bytes(O, C, taps)
    if nbytes == 0:
        raise ValueError(f"trunk_conv: C must be a multiple of 32 and the weight 3 x 3 or 1 x 1, got weight {tuple(weight.shape)}")

    def make():
        w = weight.detach().contiguous()
        packed = torch.empty(nbytes, dtype=torch.uint8, device=weight.device)
        _launch("vfa_trunk_pack_weights_f32", _lib.ptr(w), O, C, taps, _lib.ptr(packed), nbytes, _lib.current_stream_handle(), tag=(O, C, taps))
        return (packed,)
    return _conv_kept("trunk_pack", (weight,), None, weight.device, make)[0], nbytes


def trunk_conv(x, weight, stride=1, affine=None):
    """``F.conv2d(x', weight, stride=stride, padding=1)`` for a (O, C, 3, 3) weight, ``F.conv2d(x', weight, stride=stride)`` for a
    (O, C, 1, 1) weight, without bias, at inference on the HIP kernel (``vfa_trunk_conv_f32``): the raw convolution (B, O, Lo, Wo)
    contiguous.  x (B, C, L, W) float32 read through its strides, C a multiple of 32, stride 1 or 2.  ``affine = (a, b)``, both
    (B, C): ``x' = relu(a[b, c] * x + b[b, c])`` applied as the taps are read (``group_norm_affine``; the zero padding is applied to
    ``x'``); ``None``: ``x' = x``.  The three-product fp16 split of ``conv3x3`` with a per-image power-of-two scale taken after the
    prologue: the same bits on every run, alone and in a batch; no host wait, capturable."""
    a, b = (None, None) if affine is None else affine
    stride_arr, (B, C, L, W, O) = _conv_operands("trunk_conv", x, weight, a, b, kernels=(3, 1))
    if int(stride) not in (1, 2):
        raise ValueError(f"trunk_conv: stride must be 1 or 2, got {stride}")
    if affine is not None:
        if tuple(a.shape) != (B, C) or tuple(b.shape) != (B, C):
            raise ValueError(f"trunk_conv: affine must be two ({B}, {C}) tensors, got {tuple(a.shape)} and {tuple(b.shape)}")
        a, b = a.contiguous(), b.contiguous()
    taps = int(weight.shape[2]) * int(weight.shape[3])
    packed, nbytes = trunk_packed_weight(weight)
    return _trunk_conv_launch(x, stride_arr, packed, nbytes, a, b, (B, C, L, W, O), taps, int(stride))


def _trunk_conv_launch(x, stride_arr, packed, nbytes, a, b, sizes, taps, stride):
    """``vfa_trunk_conv_f32`` on checked operands and a packed weight -> (B, O, Lo, Wo) contiguous."""
    B, C, L, W, O = sizes
    Lo, Wo = ((L - 1) // stride + 1, (W - 1) // stride + 1) if L and W else (0, 0)
    out = torch.empty((B, O, Lo, Wo), dtype=torch.float32, device=x.device)
    if out.numel() == 0:
        return out
    ws_bytes = _lib.lib().vfa_trunk_workspace_bytes(B)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    _launch("vfa_trunk_conv_f32", _lib.ptr(x), stride_arr, _lib.ptr(packed), nbytes, _lib.ptr(a), _lib.ptr(b), B, C, L, W, O, taps, stride,
            _lib.ptr(out), _lib.ptr(ws), ws_bytes, _lib.current_stream_handle(), tag=(B, C, L, W, O, taps, stride))
    return out


def residual_join(y, affine, shortcut, shortcut_affine=None, out=None):
    """The end of a residual block (``vfa_residual_join_f32``): ``relu(a[b, c] * y + b[b, c] + s)`` with ``s = shortcut``, or
    ``ra[b, c] * shortcut + rb[b, c]`` with ``shortcut_affine = (ra, rb)`` -- the GroupNorm affines of ``group_norm_affine`` applied as
    the maps are read.  y and shortcut (B, C, L, W) contiguous float32, the affines (B, C); ``out``: ``None`` (a new tensor) or ``y``
    (in place).  One rounding per operation: fmaf, fmaf, add, max; a NaN stays a NaN."""
    a, b = affine
    ra, rb = (None, None) if shortcut_affine is None else shortcut_affine
    operands = (y, a, b, shortcut, ra, rb)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in operands):
        raise ValueError("residual_join: inference only -- an operand requires grad while gradients are enabled (use torch.no_grad())")
    _lib.require_device(*operands)
    if y.dtype != torch.float32 or y.dim() != 4 or shortcut.dtype != torch.float32 or shortcut.shape != y.shape:
        raise ValueError(f"residual_join: y and shortcut must be float32 (B, C, L, W) of one shape, got {tuple(y.shape)} and {tuple(shortcut.shape)}")
    if not y.is_contiguous() or not shortcut.is_contiguous():
        raise ValueError("residual_join: y and shortcut must be contiguous")
    B, C, L, W = y.shape
    for t in (a, b, ra, rb):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != (B, C)):
            raise ValueError(f"residual_join: an affine is two float32 ({B}, {C}) tensors, got {t.dtype} {tuple(t.shape)}")
    if out is not None and out is not y:
        raise ValueError("residual_join: out is None or y")
    a, b = a.contiguous(), b.contiguous()
    ra, rb = (None, None) if ra is None else (ra.contiguous(), rb.contiguous())
    out = torch.empty_like(y) if out is None else out
    if out.numel():
        _launch("vfa_residual_join_f32", _lib.ptr(y), _lib.ptr(a), _lib.ptr(b), _lib.ptr(shortcut), _lib.ptr(ra), _lib.ptr(rb), B, C, L, W,
                _lib.ptr(out), _lib.current_stream_handle(), tag=(B, C, L, W))
    return out


GN_MASK_PROLOGUE, GN_MASK_OUT = 0, 1     # VFA_GN_MASK_* of include/vfa_hip.h


def _gn_operands(name, x, groups, weight, bias):
    """What the GroupNorm wrappers ask of the shapes of a map and its parameters -> (B, C, L, W)."""
    if x.dtype != torch.float32 or x.dim() != 4 or int(groups) < 1 or x.shape[1] % int(groups):
        raise ValueError(f"{name}: the map must be float32 (B, C, L, W) with groups | C, got {x.dtype} {tuple(x.shape)}, groups {groups}")
    C = x.shape[1]
    for t in (weight, bias):
        if t is not None and (t.dtype != torch.float32 or t.numel() != C):
            raise ValueError(f"{name}: weight / bias must be float32 ({C}), got {t.dtype} {tuple(t.shape)}")
    return tuple(x.shape)


def group_norm_stats(x, groups, weight, bias, eps):
    """``group_norm_affine`` that also returns what a backward needs (``vfa_group_norm_stats_f32``) -> (a, b, stats): a and b the
    bits of ``group_norm_affine``, stats (B, groups, 2) float64, the mean and ``rstd = 1 / sqrt(var + eps)`` of each (image, group).
    The operands are read as values: no graph is recorded (``residual_block_train`` is the differentiable caller)."""
    B, C, L, W = _gn_operands("group_norm_stats", x, groups, weight, bias)
    if x.numel() == 0:
        raise ValueError("group_norm_stats: an empty map has no statistics")
    _lib.require_device(x, weight, bias)
    x = x.detach()
    weight = None if weight is None else weight.detach().contiguous()
    bias = None if bias is None else bias.detach().contiguous()
    a, b = torch.empty((B, C), dtype=torch.float32, device=x.device), torch.empty((B, C), dtype=torch.float32, device=x.device)
    stats = torch.empty((B, int(groups), 2), dtype=torch.float64, device=x.device)
    ws_bytes = _lib.lib().vfa_group_norm_workspace_bytes(B, int(groups))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    _launch("vfa_group_norm_stats_f32", _lib.ptr(x), (ctypes.c_longlong * 4)(*x.stride()), _lib.ptr(weight), _lib.ptr(bias), float(eps), B, C,
            L, W, int(groups), _lib.ptr(a), _lib.ptr(b), _lib.ptr(stats), _lib.ptr(ws), ws_bytes, _lib.current_stream_handle(),
            tag=(B, C, L, W, int(groups)))
    return a, b, stats


def group_norm_backward(u, y, a, b, weight, stats, groups, mask_out=None, want_params=True):
    """The backward of ``z = F.group_norm(y, groups, weight, bias)`` behind a ReLU, from the raw map y and ``u``, the gradient behind
    that ReLU (``vfa_group_norm_backward_f32``); a, b, stats: ``group_norm_stats(y, ...)``.  Without ``mask_out`` the ReLU is the one
    a convolution applied as it read y, ``fmaf(a, y, b) > 0`` -> (dy, dweight, dbias).  ``mask_out``: a map of y's shape whose
    positive values are the mask -- the output of a residual join -> (dy, dz, dweight, dbias) with ``dz = u`` where the mask holds
    and 0 elsewhere, the gradient of the shortcut.  ``want_params=False``: dweight and dbias are None and not computed.  float64 sums
    in a fixed order, each coefficient of ``dy = p m u + q y + r`` rounded once: the same bits on every run, and an image's dy and dz
    alone and in a batch."""
    B, C, L, W = _gn_operands("group_norm_backward", y, groups, weight, None)
    for name, t in (("u", u),) + ((("mask_out", mask_out),) if mask_out is not None else ()):
        if t.dtype != torch.float32 or tuple(t.shape) != (B, C, L, W):
            raise ValueError(f"group_norm_backward: {name} must be float32 {(B, C, L, W)} like y, got {t.dtype} {tuple(t.shape)}")
    for t in (a, b):
        if t.dtype != torch.float32 or tuple(t.shape) != (B, C):
            raise ValueError(f"group_norm_backward: the affine is two float32 ({B}, {C}) tensors, got {t.dtype} {tuple(t.shape)}")
    if stats.dtype != torch.float64 or tuple(stats.shape) != (B, int(groups), 2):
        raise ValueError(f"group_norm_backward: stats must be float64 ({B}, {int(groups)}, 2), got {stats.dtype} {tuple(stats.shape)}")
    _lib.require_device(y, u, a, b, weight, stats, mask_out)
    y, u, a, b, stats = y.detach().contiguous(), u.detach().contiguous(), a.contiguous(), b.contiguous(), stats.contiguous()
    mask_out = None if mask_out is None else mask_out.detach().contiguous()
    weight = None if weight is None else weight.detach().contiguous()
    dy = torch.empty_like(y)
    dz = torch.empty_like(y) if mask_out is not None else None
    dweight = torch.empty(C, dtype=torch.float32, device=y.device) if want_params else None
    dbias = torch.empty(C, dtype=torch.float32, device=y.device) if want_params else None
    ws_bytes = _lib.lib().vfa_group_norm_backward_workspace_bytes(B, C)
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=y.device)
    _launch("vfa_group_norm_backward_f32", _lib.ptr(y), _lib.ptr(u), _lib.ptr(a), _lib.ptr(b), _lib.ptr(mask_out), _lib.ptr(weight),
            _lib.ptr(stats), GN_MASK_PROLOGUE if mask_out is None else GN_MASK_OUT, B, C, L, W, int(groups), _lib.ptr(dy), _lib.ptr(dz),
            _lib.ptr(dweight), _lib.ptr(dbias), _lib.ptr(ws), ws_bytes, _lib.current_stream_handle(), tag=(B, C, L, W, int(groups)))
    return (dy, dweight, dbias) if mask_out is None else (dy, dz, dweight, dbias)


def _trunk_grad_operands(name, grad, weight):
    if weight.dtype != torch.float32 or weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3) or weight.shape[0] % 32 or weight.shape[1] % 32:
        raise ValueError(f"{name}: weight must be float32 (O, C, 3, 3) with O and C multiples of 32, got {weight.dtype} {tuple(weight.shape)}")
    if grad.dtype != torch.float32 or grad.dim() != 4 or grad.shape[1] != weight.shape[0]:
        raise ValueError(f"{name}: grad must be float32 (B, {weight.shape[0]}, L, W), got {grad.dtype} {tuple(grad.shape)}")
    _lib.require_device(grad, weight)


def trunk_conv_input_grad(grad, weight):
    """dL/dx' of ``y = F.conv2d(x', weight, padding=1)`` (``trunk_conv`` at stride 1) from grad = dL/dy (B, O, L, W), read through its
    strides: ``vfa_trunk_conv_f32`` on ``grad`` with the planes of the transposed, tap-mirrored weight, packed per call from ``weight``
    (O, C, 3, 3) as it lies and kept nowhere -> (B, C, L, W) contiguous; two accumulator chains where O > 256.  An image gives the
    same bits alone and in a batch."""
    _trunk_grad_operands("trunk_conv_input_grad", grad, weight)
    O, C = int(weight.shape[0]), int(weight.shape[1])
    B, _, L, W = grad.shape
    grad = grad.detach()
    packed, nbytes = _conv3x3_pack(weight, transposed=True)
    return _trunk_conv_launch(grad, (ctypes.c_longlong * 4)(*grad.stride()), packed, nbytes, None, None, (B, O, L, W, C), 9, 1)


def trunk_conv_weight_grad(grad, x, affine=None):
    """dL/dweight (O, C, 3, 3) of ``y = F.conv2d(x', weight, padding=1)`` from grad = dL/dy (B, O, L, W) and x (B, C, L, W), both read
    through their strides (``vfa_trunk_conv_wgrad_f32``).  ``affine = (a, b)``, both (B, C): ``x' = relu(a[b, c] * x + b[b, c])``
    applied as x is read (the zero padding is applied to ``x'``), its power-of-two scale taken after that; ``None``: ``x' = x``.  O
    and C multiples of 32.  The kernels of ``conv3x3_weight_grad`` with the slabs of ``slabs_for`` (``csrc/vfa_conv_grad.h``): up to
    O C = 256^2 its slabs -- and without an affine its bits --, fewer past it, so the partials of a 512 x 512 layer are a quarter of
    what they would be.  The same bits on every run."""
    a, b = (None, None) if affine is None else affine
    if x.dtype != torch.float32 or x.dim() != 4 or grad.dtype != torch.float32 or grad.dim() != 4 or grad.shape[0] != x.shape[0] \
            or grad.shape[2:] != x.shape[2:]:
        raise ValueError(f"trunk_conv_weight_grad: grad (B, O, L, W) and x (B, C, L, W) must be float32 maps of one size, got "
                         f"{grad.dtype} {tuple(grad.shape)} and {x.dtype} {tuple(x.shape)}")
    B, C, L, W = x.shape
    O = int(grad.shape[1])
    if C % 32 or O % 32 or not C or not O:
        raise ValueError(f"trunk_conv_weight_grad: C and O must be multiples of 32, got {C} and {O}")
    if affine is not None:
        if any(t.dtype != torch.float32 or tuple(t.shape) != (B, C) for t in (a, b)):
            raise ValueError(f"trunk_conv_weight_grad: affine must be two float32 ({B}, {C}) tensors, got {tuple(a.shape)} and {tuple(b.shape)}")
        a, b = a.contiguous(), b.contiguous()
    _lib.require_device(grad, x, a, b)
    grad, x = grad.detach(), x.detach()
    dw = torch.empty((O, C, 3, 3), dtype=torch.float32, device=x.device)
    ws_bytes = _lib.lib().vfa_trunk_conv_wgrad_workspace_bytes(B, O, C, L, W)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=x.device)
    _launch("vfa_trunk_conv_wgrad_f32", _lib.ptr(grad), (ctypes.c_longlong * 4)(*grad.stride()), _lib.ptr(x), (ctypes.c_longlong * 4)(*x.stride()),
            _lib.ptr(a), _lib.ptr(b), B, C, L, W, O, _lib.ptr(dw), _lib.ptr(ws), ws_bytes, _lib.current_stream_handle(),
            tag=(B, C, L, W, O, affine is not None))
    return dw


def residual_block_workspace_bytes(B, C, L, W):
    """The largest transient workspace of one ``residual_block_train`` step on a (B, C, L, W) map: the weight gradient's partials."""
    return int(_lib.lib().vfa_trunk_conv_wgrad_workspace_bytes(B, C, C, L, W))


class _ResidualBlockTrain(torch.autograd.Function):
    """``residual_block_train``: one node for the whole identity block -- the affines are functions of y1 and y2, so smaller
    differentiable pieces do not compose.  Three maps are kept besides the input (y1, y2 and the join); the normalised maps are
    recomputed in prologues.  The packed planes are made per call and kept nowhere: a weight under training changes every step."""

    @staticmethod
    def forward(ctx, x, w1, g1, b1, w2, g2, b2, groups, eps):
        B, C, L, W = x.shape
        x = x.detach().contiguous()
        sizes = (B, C, L, W, C)

        def conv(t, w, a=None, b=None):
            packed, nbytes = _conv3x3_pack(w)
            return _trunk_conv_launch(t, (ctypes.c_longlong * 4)(*t.stride()), packed, nbytes, a, b, sizes, 9, 1)
        y1 = conv(x, w1)
        a1, c1, s1 = group_norm_stats(y1, groups, g1, b1, eps)
        y2 = conv(y1, w2, a1, c1)
        a2, c2, s2 = group_norm_stats(y2, groups, g2, b2, eps)
        out = residual_join(y2, (a2, c2), x)
        ctx.save_for_backward(x, y1, y2, out, a1, c1, s1, a2, c2, s2, w1, g1, w2, g2)
        ctx.groups = groups
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        x, y1, y2, out, a1, c1, s1, a2, c2, s2, w1, g1, w2, g2 = ctx.saved_tensors
        need = ctx.needs_input_grad
        dw1 = dg1 = db1 = dw2 = dg2 = db2 = dx = None
        dy2, dz, dg2, db2 = group_norm_backward(grad, y2, a2, c2, g2, s2, ctx.groups, mask_out=out, want_params=need[5] or need[6])
        if need[4]:
            dw2 = trunk_conv_weight_grad(dy2, y1, (a1, c1))
        if any(need[:4]):
            dx1 = trunk_conv_input_grad(dy2, w2)
            del dy2
            dy1, dg1, db1 = group_norm_backward(dx1, y1, a1, c1, g1, s1, ctx.groups, want_params=need[2] or need[3])
            del dx1
            if need[1]:
                dw1 = trunk_conv_weight_grad(dy1, x)
            if need[0]:
                dx = trunk_conv_input_grad(dy1, w1).add_(dz)       # one elementwise add, the convolution term first
        return (dx, dw1, dg1 if need[2] else None, db1 if need[3] else None, dw2, dg2 if need[5] else None, db2 if need[6] else None,
                None, None)


def residual_block_train(x, w1, g1, b1, w2, g2, b2, groups=16, eps=1e-5):
    """An identity residual block of the trunk with gradients, on the HIP kernels: ``relu(gn2(conv2(relu(gn1(conv1(x))))) + x)`` with
    3 x 3 convolutions of stride 1 without bias (w1, w2: (C, C, 3, 3), C a multiple of 32) and GroupNorms of ``groups`` groups (g, b:
    (C) weights and biases), x (B, C, L, W) float32 -> (B, C, L, W) contiguous, the bits of ``_Block.forward_hip`` under ``no_grad``.
    ONE once-differentiable node.  Forward: ``trunk_conv``, ``group_norm_stats``, ``trunk_conv`` with the affine as its prologue,
    ``group_norm_stats``, ``residual_join``; x, the two raw maps, the join, the affines and the statistics are saved.  Backward:
    ``group_norm_backward`` with the join's mask (-> dy2 and the shortcut's dz), ``trunk_conv_weight_grad`` with the first affine as
    its prologue, ``trunk_conv_input_grad``, ``group_norm_backward`` with the prologue's mask, ``trunk_conv_weight_grad``,
    ``trunk_conv_input_grad`` + dz -- only what ``needs_input_grad`` asks for.  Fixed summation order, no float atomics: the same
    bits on every run without ``torch.use_deterministic_algorithms``, and an image's dx alone and in a batch; no host wait, capturable."""
    if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] % 32 or x.numel() == 0:
        raise ValueError(f"residual_block_train: x must be a float32 (B, C, L, W) map with values and C a multiple of 32, got {x.dtype} {tuple(x.shape)}")
    C = int(x.shape[1])
    if int(groups) < 1 or C % int(groups):
        raise ValueError(f"residual_block_train: groups must divide C = {C}, got {groups}")
    for w in (w1, w2):
        if w.dtype != torch.float32 or tuple(w.shape) != (C, C, 3, 3):
            raise ValueError(f"residual_block_train: a weight must be float32 ({C}, {C}, 3, 3), got {w.dtype} {tuple(w.shape)}")
    for t in (g1, b1, g2, b2):
        if t.dtype != torch.float32 or tuple(t.shape) != (C,):
            raise ValueError(f"residual_block_train: a GroupNorm parameter must be float32 ({C},), got {t.dtype} {tuple(t.shape)}")
    _lib.require_device(x, w1, g1, b1, w2, g2, b2)
    return _ResidualBlockTrain.apply(x, w1, g1, b1, w2, g2, b2, int(groups), float(eps))


def _down_size(n):
    return (n - 1) // 2 + 1 if n else 0


def trunk_down_weight_grad(grad, x, kernel):
    """dL/dweight of a stride-2 convolution of the trunk (``vfa_trunk_down_wgrad_f32``): ``kernel`` 3 for ``y = F.conv2d(x, weight,
    stride=2, padding=1)`` -> (O, C, 3, 3), 1 for ``y = F.conv2d(x, weight, stride=2)`` -> (O, C, 1, 1); grad = dL/dy (B, O, Lo, Wo)
    with ``Lo = (L - 1) // 2 + 1``, x (B, C, L, W), both float32 and read through their strides, O and C multiples of 32.  The
    kernels of ``trunk_conv_weight_grad`` on K tiles of 2 x 32 cells, ``slabs_for(Lo, Wo, O, C)`` slabs merged in float64 in ascending
    order: the same bits on every run."""
    if int(kernel) not in (3, 1):
        raise ValueError(f"trunk_down_weight_grad: kernel must be 3 or 1, got {kernel}")
    if x.dtype != torch.float32 or x.dim() != 4 or grad.dtype != torch.float32 or grad.dim() != 4 or grad.shape[0] != x.shape[0] \
            or tuple(grad.shape[2:]) != (_down_size(x.shape[2]), _down_size(x.shape[3])):
        raise ValueError(f"trunk_down_weight_grad: grad (B, O, Lo, Wo) and x (B, C, L, W) must be float32 maps with (Lo, Wo) the stride-2 "
                         f"size of (L, W), got {grad.dtype} {tuple(grad.shape)} and {x.dtype} {tuple(x.shape)}")
    B, C, L, W = x.shape
    O = int(grad.shape[1])
    if C % 32 or O % 32 or not C or not O:
        raise ValueError(f"trunk_down_weight_grad: C and O must be multiples of 32, got {C} and {O}")
    _lib.require_device(grad, x)
    grad, x, k = grad.detach(), x.detach(), int(kernel)
    dw = torch.empty((O, C, k, k), dtype=torch.float32, device=x.device)
    ws_bytes = _lib.lib().vfa_trunk_down_wgrad_workspace_bytes(B, O, C, L, W, k)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=x.device)
    _launch("vfa_trunk_down_wgrad_f32", _lib.ptr(grad), (ctypes.c_longlong * 4)(*grad.stride()), _lib.ptr(x), (ctypes.c_longlong * 4)(*x.stride()),
            B, C, L, W, O, k, _lib.ptr(dw), _lib.ptr(ws), ws_bytes, _lib.current_stream_handle(), tag=(B, C, L, W, O, k))
    return dw


def trunk_down_input_grad(grad, weight, size, add_to=None):
    """dL/dx of a stride-2 convolution of the trunk (``vfa_trunk_down_dgrad_f32``) from grad = dL/dy (B, O, Lo, Wo), read through its
    strides, and ``weight`` (O, C, 3, 3) (padding 1) or (O, C, 1, 1) as it lies; ``size = (L, W)`` of x, which stride 2 does not
    determine: ``(L - 1) // 2 + 1`` must be Lo -> (B, C, L, W) contiguous.  The four parity classes of dx are four launches of the
    dense kernel over their own 1, 2, 2 and 4 taps; every element is written exactly once; an image gives the same bits alone and in a
    batch.  ``add_to``: a contiguous (B, C, L, W) map to which the gradient is added in place, ``add_to + gradient`` in that order
    (returned) -- the only form a 1 x 1 weight has, whose gradient touches the even positions alone."""
    if weight.dtype != torch.float32 or weight.dim() != 4 or tuple(weight.shape[2:]) not in ((3, 3), (1, 1)) or weight.shape[0] % 32 \
            or weight.shape[1] % 32:
        raise ValueError(f"trunk_down_input_grad: weight must be float32 (O, C, 3, 3) or (O, C, 1, 1) with O and C multiples of 32, got "
                         f"{weight.dtype} {tuple(weight.shape)}")
    O, C, k = int(weight.shape[0]), int(weight.shape[1]), int(weight.shape[2])
    L, W = (int(v) for v in size)
    if grad.dtype != torch.float32 or grad.dim() != 4 or tuple(grad.shape[1:]) != (O, _down_size(L), _down_size(W)) or L < 1 or W < 1:
        raise ValueError(f"trunk_down_input_grad: grad must be float32 (B, {O}, {_down_size(L)}, {_down_size(W)}) for size {(L, W)}, got "
                         f"{grad.dtype} {tuple(grad.shape)}")
    B = int(grad.shape[0])
    if add_to is None and k == 1:
        raise ValueError("trunk_down_input_grad: the gradient of a 1 x 1 weight is added to a map (add_to)")
    if add_to is not None and (add_to.dtype != torch.float32 or tuple(add_to.shape) != (B, C, L, W) or not add_to.is_contiguous()):
        raise ValueError(f"trunk_down_input_grad: add_to must be a contiguous float32 {(B, C, L, W)} map, got {add_to.dtype} {tuple(add_to.shape)}")
    _lib.require_device(grad, weight, add_to)
    grad, w = grad.detach(), weight.detach().contiguous()
    dx = torch.empty((B, C, L, W), dtype=torch.float32, device=grad.device) if add_to is None else add_to
    if dx.numel() == 0:
        return dx
    ws_bytes = _lib.lib().vfa_trunk_down_dgrad_workspace_bytes(B, O, C, k)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=grad.device)
    _launch("vfa_trunk_down_dgrad_f32", _lib.ptr(grad), (ctypes.c_longlong * 4)(*grad.stride()), _lib.ptr(w), B, O, int(grad.shape[2]),
            int(grad.shape[3]), C, L, W, k, int(add_to is not None), _lib.ptr(dx), _lib.ptr(ws), ws_bytes, _lib.current_stream_handle(),
            tag=(B, O, C, L, W, k, add_to is not None))
    return dx


class _ProjectionBlockTrain(torch.autograd.Function):
    """``projection_block_train``: one node for the whole projection block, like ``_ResidualBlockTrain``.  Four maps are kept
    besides the input (y1, y2, yd and the join); the packed planes are made per call and kept nowhere."""

    @staticmethod
    def forward(ctx, x, w1, g1, b1, w2, g2, b2, wd, gd, bd, groups, eps):
        B, C, L, W = x.shape
        O = int(w1.shape[0])
        x = x.detach().contiguous()
        Lo, Wo = _down_size(L), _down_size(W)

        def conv(t, w, sizes, stride, a=None, b=None):
            taps = int(w.shape[2]) * int(w.shape[3])
            nbytes = _lib.lib().vfa_trunk_packed_bytes(int(w.shape[0]), int(w.shape[1]), taps)
            packed = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
            _launch("vfa_trunk_pack_weights_f32", _lib.ptr(w.detach().contiguous()), int(w.shape[0]), int(w.shape[1]), taps, _lib.ptr(packed), nbytes,
                    _lib.current_stream_handle(), tag=(int(w.shape[0]), int(w.shape[1]), taps))
            return _trunk_conv_launch(t, (ctypes.c_longlong * 4)(*t.stride()), packed, nbytes, a, b, sizes, taps, stride)
        y1 = conv(x, w1, (B, C, L, W, O), 2)
        a1, c1, s1 = group_norm_stats(y1, groups, g1, b1, eps)
        y2 = conv(y1, w2, (B, O, Lo, Wo, O), 1, a1, c1)
        a2, c2, s2 = group_norm_stats(y2, groups, g2, b2, eps)
        yd = conv(x, wd, (B, C, L, W, O), 2)
        ad, cd, sd = group_norm_stats(yd, groups, gd, bd, eps)
        out = residual_join(y2, (a2, c2), yd, (ad, cd))
        ctx.save_for_backward(x, y1, y2, yd, out, a1, c1, s1, a2, c2, s2, ad, cd, sd, w1, g1, w2, g2, wd, gd)
        ctx.groups = groups
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        x, y1, y2, yd, out, a1, c1, s1, a2, c2, s2, ad, cd, sd, w1, g1, w2, g2, wd, gd = ctx.saved_tensors
        need = ctx.needs_input_grad
        dx = dw1 = dg1 = db1 = dw2 = dwd = None
        dy2, dz, dg2, db2 = group_norm_backward(grad, y2, a2, c2, g2, s2, ctx.groups, mask_out=out, want_params=need[5] or need[6])
        dyd = dgd = dbd = None
        if need[0] or any(need[7:10]):
            # the projection's GroupNorm sits behind the same ReLU: u = dz, and m ? dz : 0 is dz bit for bit (the second dz is dropped)
            dyd, _, dgd, dbd = group_norm_backward(dz, yd, ad, cd, gd, sd, ctx.groups, mask_out=out, want_params=need[8] or need[9])
        del dz
        if need[4]:
            dw2 = trunk_conv_weight_grad(dy2, y1, (a1, c1))
        if need[7]:
            dwd = trunk_down_weight_grad(dyd, x, 1)
        if any(need[:4]):
            dx1 = trunk_conv_input_grad(dy2, w2)
            del dy2
            dy1, dg1, db1 = group_norm_backward(dx1, y1, a1, c1, g1, s1, ctx.groups, want_params=need[2] or need[3])
            del dx1
            if need[1]:
                dw1 = trunk_down_weight_grad(dy1, x, 3)
            if need[0]:
                dx = trunk_down_input_grad(dy1, w1, x.shape[2:])               # the 3 x 3 term first,
                dx = trunk_down_input_grad(dyd, wd, x.shape[2:], add_to=dx)   # then the projection's, added to it
        return (dx, dw1, dg1 if need[2] else None, db1 if need[3] else None, dw2, dg2 if need[5] else None, db2 if need[6] else None,
                dwd, dgd if need[8] else None, dbd if need[9] else None, None, None)


def projection_block_train(x, w1, g1, b1, w2, g2, b2, wd, gd, bd, groups=16, eps=1e-5):
    """A projection block of the trunk with gradients, on the HIP kernels: ``relu(gn2(conv2(relu(gn1(conv1(x))))) + gnd(convd(x)))``
    with ``conv1`` 3 x 3 of stride 2 (w1: (O, C, 3, 3)), ``conv2`` 3 x 3 of stride 1 (w2: (O, O, 3, 3)), ``convd`` 1 x 1 of stride 2
    (wd: (O, C, 1, 1)), all without bias, C and O multiples of 32, and GroupNorms of ``groups`` groups (g, b: (O)); x (B, C, L, W)
    float32 -> (B, O, Lo, Wo) contiguous with ``Lo = (L - 1) // 2 + 1``, the bits of ``_Block.forward_hip`` under ``no_grad``.  ONE
    once-differentiable node.  Forward: the calls of ``forward_hip`` with ``group_norm_stats`` and a join that is not in place; x, the
    three raw maps, the join, the affines and the statistics are saved -- four maps besides the input.  Backward:
    ``group_norm_backward`` with the join's mask (-> dy2 and dz), the same entry point once more on (dz, yd) for the projection's
    GroupNorm, ``trunk_conv_weight_grad`` / ``trunk_conv_input_grad`` / ``group_norm_backward`` for conv2 and the first GroupNorm as in
    ``residual_block_train``, ``trunk_down_weight_grad`` for w1 and wd, and dx = ``trunk_down_input_grad`` of (dy1, w1), then that of
    (dyd, wd) added to it -- only what ``needs_input_grad`` asks for.  Fixed summation order, no float atomics: the same bits on every
    run without ``torch.use_deterministic_algorithms``, and an image's dx alone and in a batch; no host wait, capturable."""
    if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] % 32 or x.numel() == 0:
        raise ValueError(f"projection_block_train: x must be a float32 (B, C, L, W) map with values and C a multiple of 32, got {x.dtype} {tuple(x.shape)}")
    C = int(x.shape[1])
    O = int(w1.shape[0]) if w1.dim() == 4 else 0
    if O < 1 or O % 32:
        raise ValueError(f"projection_block_train: O must be a multiple of 32, got w1 {tuple(w1.shape)}")
    if int(groups) < 1 or O % int(groups):
        raise ValueError(f"projection_block_train: groups must divide O = {O}, got {groups}")
    for w, shape in ((w1, (O, C, 3, 3)), (w2, (O, O, 3, 3)), (wd, (O, C, 1, 1))):
        if w.dtype != torch.float32 or tuple(w.shape) != shape:
            raise ValueError(f"projection_block_train: a weight must be float32 {shape}, got {w.dtype} {tuple(w.shape)}")
    for t in (g1, b1, g2, b2, gd, bd):
        if t.dtype != torch.float32 or tuple(t.shape) != (O,):
            raise ValueError(f"projection_block_train: a GroupNorm parameter must be float32 ({O},), got {t.dtype} {tuple(t.shape)}")
    _lib.require_device(x, w1, g1, b1, w2, g2, b2, wd, gd, bd)
    return _ProjectionBlockTrain.apply(x, w1, g1, b1, w2, g2, b2, wd, gd, bd, int(groups), float(eps))


_STEM_MAX_OUT = 64      # kMaxOut of csrc/vfa_stem.h


def stem_conv(x, weight):
    """``F.conv2d(x, weight, stride=2, padding=3)`` for a (O, 3, 7, 7) weight with at most 64 outputs, without bias, at inference on the
    HIP kernel (``vfa_stem_conv_f32``): the raw map (B, O, (L - 1) // 2 + 1, (W - 1) // 2 + 1) contiguous.  x (B, 3, L, W) float32 is read
    through its strides (NCHW, channels-last or a slice, never copied).  The exact f32 MFMA: per output one ``fmaf`` chain over
    k = (c * 7 + ky) * 7 + kx ascending, a tap outside the image being a zero operand -- no scales, no pre-pass: the same bits on
    every run, alone and in a batch; no host wait, capturable.  Nothing is kept between calls."""
    stride_arr, (B, C, L, W, O) = _conv_operands("stem_conv", x, weight, kernels=(7,))
    if C != 3 or O > _STEM_MAX_OUT:
        raise ValueError(f"stem_conv: weight must be (O, 3, 7, 7) with O <= {_STEM_MAX_OUT}, got {tuple(weight.shape)}")
    w = weight.detach().contiguous()
    Lo, Wo = ((L - 1) // 2 + 1, (W - 1) // 2 + 1) if L and W else (0, 0)
    out = torch.empty((B, O, Lo, Wo), dtype=torch.float32, device=x.device)
    if out.numel() == 0:
        return out
    ws_bytes = _lib.lib().vfa_stem_workspace_bytes(O)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    _launch("vfa_stem_conv_f32", _lib.ptr(x), stride_arr, _lib.ptr(w), B, C, L, W, O, _lib.ptr(out), _lib.ptr(ws), ws_bytes,
            _lib.current_stream_handle(), tag=(B, C, L, W, O))
    return out


def stem_pool(y, affine):
    """``F.max_pool2d(relu(a[b, c] * y + b[b, c]), 3, stride=2, padding=1)`` at inference (``vfa_stem_pool_f32``): y (B, C, L, W)
    contiguous float32, ``affine = (a, b)``, both (B, C) (``group_norm_affine`` on y: GroupNorm and the ReLU applied as the taps are
    read) -> (B, C, (L - 1) // 2 + 1, (W - 1) // 2 + 1).  Each tap is ``max(fmaf(a, y, b), 0)``, one rounding; taps outside the map are
    skipped; a NaN reaches exactly the cells whose window holds it."""
    a, b = affine
    if torch.is_grad_enabled() and any(t.requires_grad for t in (y, a, b)):
        raise ValueError("stem_pool: inference only -- an operand requires grad while gradients are enabled (use torch.no_grad())")
    _lib.require_device(y, a, b)
    if y.dtype != torch.float32 or y.dim() != 4 or not y.is_contiguous():
        raise ValueError(f"stem_pool: y must be contiguous float32 (B, C, L, W), got {y.dtype} {tuple(y.shape)}")
    B, C, L, W = y.shape
    for t in (a, b):
        if t.dtype != torch.float32 or tuple(t.shape) != (B, C):
            raise ValueError(f"stem_pool: the affine is two float32 ({B}, {C}) tensors, got {t.dtype} {tuple(t.shape)}")
    a, b = a.contiguous(), b.contiguous()
    Lo, Wo = ((L - 1) // 2 + 1, (W - 1) // 2 + 1) if L and W else (0, 0)
    out = torch.empty((B, C, Lo, Wo), dtype=torch.float32, device=y.device)
    if out.numel():
        _launch("vfa_stem_pool_f32", _lib.ptr(y), _lib.ptr(a), _lib.ptr(b), B, C, L, W, _lib.ptr(out), _lib.current_stream_handle(),
                tag=(B, C, L, W))
    return out


def stem_pool_backward(gout, y, affine):
    """The backward of ``stem_pool`` up to, but not through, the ReLU (``vfa_stem_pool_backward_f32``): gout (B, C, Lo, Wo), the
    gradient of the pooled map, y (B, C, L, W) the raw map and ``affine = (a, b)`` the forward's -> u (B, C, L, W) contiguous,
    ``u[b, c, p, q]`` the sum of gout over the windows whose winning tap is (p, q), in ascending window order from +0.  The taps are
    recomputed with the forward's bits and the winner is the forward's: the first of equal maxima, the last NaN.  The ReLU's mask
    is not applied -- u is the gradient behind the ReLU that ``group_norm_backward`` expects.  A gather, no atomics: the same bits
    on every run, and an image alone and in a batch."""
    a, b = affine
    _lib.require_device(gout, y, a, b)
    if y.dtype != torch.float32 or y.dim() != 4:
        raise ValueError(f"stem_pool_backward: y must be float32 (B, C, L, W), got {y.dtype} {tuple(y.shape)}")
    B, C, L, W = y.shape
    Lo, Wo = (_down_size(L), _down_size(W)) if L and W else (0, 0)
    if gout.dtype != torch.float32 or tuple(gout.shape) != (B, C, Lo, Wo):
        raise ValueError(f"stem_pool_backward: gout must be float32 {(B, C, Lo, Wo)}, got {gout.dtype} {tuple(gout.shape)}")
    for t in (a, b):
        if t.dtype != torch.float32 or tuple(t.shape) != (B, C):
            raise ValueError(f"stem_pool_backward: the affine is two float32 ({B}, {C}) tensors, got {t.dtype} {tuple(t.shape)}")
    gout, y, a, b = gout.detach().contiguous(), y.detach().contiguous(), a.detach().contiguous(), b.detach().contiguous()
    u = torch.empty_like(y)
    if u.numel():
        _launch("vfa_stem_pool_backward_f32", _lib.ptr(gout), _lib.ptr(y), _lib.ptr(a), _lib.ptr(b), B, C, L, W, _lib.ptr(u),
                _lib.current_stream_handle(), tag=(B, C, L, W))
    return u


def stem_conv_weight_grad(grad, x):
    """dL/dweight (O, 3, 7, 7) of ``y = F.conv2d(x, weight, stride=2, padding=3)`` (``stem_conv``) from grad = dL/dy
    (B, O, (L - 1) // 2 + 1, (W - 1) // 2 + 1) and the images x (B, 3, L, W), read through their strides and never copied
    (``vfa_stem_conv_wgrad_f32``), O <= 64.  The exact f32 MFMA with the output cells as K; slabs of ``wgrad_slabs(Lo, Wo)``
    (``csrc/vfa_stem.h``), one float32 partial per (image, slab), merged in float64 in ascending order and rounded once: the same
    bits on every run; integer-valued operands give float64's result exactly.  No host wait, capturable."""
    _lib.require_device(grad, x)
    if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"stem_conv_weight_grad: x must be float32 (B, 3, L, W), got {x.dtype} {tuple(x.shape)}")
    B, _, L, W = x.shape
    Lo, Wo = (_down_size(L), _down_size(W)) if L and W else (0, 0)
    if grad.dtype != torch.float32 or grad.dim() != 4 or grad.shape[0] != B or tuple(grad.shape[2:]) != (Lo, Wo) \
            or not 1 <= grad.shape[1] <= _STEM_MAX_OUT:
        raise ValueError(f"stem_conv_weight_grad: grad must be float32 ({B}, O <= {_STEM_MAX_OUT}, {Lo}, {Wo}), got {grad.dtype} {tuple(grad.shape)}")
    O = int(grad.shape[1])
    grad, x = grad.detach().contiguous(), x.detach()
    dw = torch.empty((O, 3, 7, 7), dtype=torch.float32, device=x.device)
    ws_bytes = _lib.lib().vfa_stem_conv_wgrad_workspace_bytes(B, O, L, W)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=x.device)
    _launch("vfa_stem_conv_wgrad_f32", _lib.ptr(grad), _lib.ptr(x), (ctypes.c_longlong * 4)(*x.stride()), B, L, W, O, _lib.ptr(dw), _lib.ptr(ws),
            ws_bytes, _lib.current_stream_handle(), tag=(B, L, W, O))
    return dw


class _StemTrain(torch.autograd.Function):
    """``stem_train``: one node for the whole stem.  Besides the images only the raw map is kept; the normalised map is never
    written and the pooling keeps no index map -- its winners are recomputed from the raw map in the backward."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, groups, eps):
        x = x.detach()
        y = stem_conv(x, weight)
        a, b, stats = group_norm_stats(y, groups, gamma, beta, eps)
        out = stem_pool(y, (a, b))
        ctx.save_for_backward(x, y, a, b, stats, gamma, weight)
        ctx.groups = groups
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        x, y, a, b, stats, gamma, weight = ctx.saved_tensors
        need = ctx.needs_input_grad
        dw = dgamma = dbeta = None
        if any(need[1:4]):
            u = stem_pool_backward(grad, y, (a, b))
            dy, dgamma, dbeta = group_norm_backward(u, y, a, b, gamma, stats, ctx.groups, want_params=need[2] or need[3])
            del u
            if need[1]:
                dw = stem_conv_weight_grad(dy, x)
        return None, dw, dgamma if need[2] else None, dbeta if need[3] else None, None, None


def stem_train(x, weight, gamma, beta, groups=16, eps=1e-5):
    """The trunk's stem with gradients, on the HIP kernels: ``max_pool2d(relu(group_norm(conv2d(x, weight, stride=2, padding=3))), 3,
    2, 1)`` with weight (O, 3, 7, 7), O <= 64, without bias, and a GroupNorm of ``groups`` groups (gamma, beta: (O)); x (B, 3, L, W)
    float32, read through its strides -> the pooled map, contiguous, the bits of ``_Trunk.stem_hip`` under ``no_grad``.  ONE
    once-differentiable node.  Forward: ``stem_conv``, ``group_norm_stats``, ``stem_pool``; x, the raw map, the affine, the
    statistics, gamma and the weight are saved -- one map besides the images.  Backward: ``stem_pool_backward`` (-> u),
    ``group_norm_backward`` with the prologue's mask (-> dy, dgamma, dbeta), ``stem_conv_weight_grad`` -- only what
    ``needs_input_grad`` asks for.  The images are data: an x that requires grad raises ``ValueError``.  Fixed summation order, no
    float atomics: the same bits on every run without ``torch.use_deterministic_algorithms``; no host wait, capturable."""
    if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3 or x.numel() == 0:
        raise ValueError(f"stem_train: x must be a float32 (B, 3, L, W) batch with values, got {x.dtype} {tuple(x.shape)}")
    if x.requires_grad:
        raise ValueError("stem_train: x requires grad, and the stem has no input gradient (the images are data)")
    if weight.dtype != torch.float32 or weight.dim() != 4 or tuple(weight.shape[1:]) != (3, 7, 7) or not 1 <= weight.shape[0] <= _STEM_MAX_OUT:
        raise ValueError(f"stem_train: weight must be float32 (O <= {_STEM_MAX_OUT}, 3, 7, 7), got {weight.dtype} {tuple(weight.shape)}")
    O = int(weight.shape[0])
    if int(groups) < 1 or O % int(groups):
        raise ValueError(f"stem_train: groups must divide O = {O}, got {groups}")
    for t in (gamma, beta):
        if t.dtype != torch.float32 or tuple(t.shape) != (O,):
            raise ValueError(f"stem_train: a GroupNorm parameter must be float32 ({O},), got {t.dtype} {tuple(t.shape)}")
    _lib.require_device(x, weight, gamma, beta)
    return _StemTrain.apply(x, weight, gamma, beta, int(groups), float(eps))
