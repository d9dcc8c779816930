"""Which driver a frame runs through, for every switch, layer count, camera count and gradient state (no GPU).

Part A drives the public entry points (``aggregate_views`` with laterals, ``integrals=`` and ``frames=``, ``VFA.forward``,
``vfa_op._materialize``) with CPU tensors while the drivers are spies, and compares what ran with
``tests/golden/frame_route_parent.json``: the observations recorded on the commit before ``vfa_op.frame_route`` existed
(``python tests/test_frame_route_cpu.py`` writes the file anew from the code it is run on).  Part B asserts that ``frame_route`` names,
for every row of part A, the driver that part A observed.
"""
import itertools
import json
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # (when run as a script)
GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frame_route_parent.json")

L, W = 8, 8
DEFAULTS = dict(PIPE=True, PIPE_SINGLE_LAYER=False, FUSED_POOL=True, WINDOW_POOL=True, COLLAPSE_KERNEL="mfma_bf16", FUSED_TRAIN=True,
                VOX_BYTES_LIMIT=8 << 30)
SWITCHES = {
    "default": {},
    "pipe_off": dict(PIPE=False),
    "pipe_single_layer": dict(PIPE_SINGLE_LAYER=True),
    "fused_pool_off": dict(FUSED_POOL=False),
    "fused_window_off": dict(FUSED_POOL=False, WINDOW_POOL=False),
    "library": dict(COLLAPSE_KERNEL="library"),
    "fused_train_off": dict(FUSED_TRAIN=False),
    "pipe_fused_off": dict(PIPE=False, FUSED_POOL=False),
    # the transient voxel buffer of 7 cameras on the 8 x 8 grid is 7 * 64 * 1024 bytes: one byte less and "window" gives way
    "vox_fits": dict(FUSED_POOL=False, VOX_BYTES_LIMIT=7 * L * W * 1024),
    "vox_too_small": dict(FUSED_POOL=False, VOX_BYTES_LIMIT=7 * L * W * 1024 - 1),
}
GRID_SWITCHES = [s for s in SWITCHES if not s.startswith("vox_")]
GRADS = ("off", "weights", "lateral", "calibs")
# route -> the drivers one frame of three scales calls
DRIVERS = {"zeros": "", "train": "fused_frame_train", "pipe_batch": "pipe_frames", "pipe": "pipe_frame", "fused": "fused_frame",
           "window": "window_frame", "scale_mfma": "project_sum,project_sum,project_sum",
           "scale_autograd": "project_views,project_views,project_views"}


def _rows():
    rows = []
    for nl, n, grad, kind, sw in itertools.product((1, 5), (0, 1, 7, 32, 33), GRADS, ("laterals", "integrals"), GRID_SWITCHES):
        rows.append(dict(entry="aggregate", nl=nl, n=n, grad=grad, kind=kind, sw=sw, mods="same"))
    for sw in ("vox_fits", "vox_too_small"):
        rows.append(dict(entry="aggregate", nl=1, n=7, grad="off", kind="laterals", sw=sw, mods="same"))
    for breaker, grad, kind in itertools.product(("c128", "layers", "image_size"), ("off", "weights"), ("laterals", "integrals")):
        rows.append(dict(entry="aggregate", nl=1, n=7, grad=grad, kind=kind, sw="default", mods=breaker))
    for nl, kind, sw, variant in itertools.product((1, 5), ("laterals", "integrals"), GRID_SWITCHES, ("one_rig", "rig_per_frame", "grads")):
        rows.append(dict(entry="frames", nl=nl, n=7, grad="weights" if variant == "grads" else "off", kind=kind, sw=sw, mods="same",
                         variant=variant))
    for nl, grad, sw in itertools.product((1, 5), GRADS, GRID_SWITCHES):
        rows.append(dict(entry="forward", nl=nl, n=1, grad=grad, kind="laterals", sw=sw, mods="same"))
    for nl, n, sw, cameras in itertools.product((1, 5), (1, 7, 33), GRID_SWITCHES, ("same_cameras", "other_cameras")):
        rows.append(dict(entry="materialize", nl=nl, n=n, grad="off", kind="laterals", sw=sw, mods="same", variant=cameras))
    return rows


def _row_id(r):
    return "-".join(str(r[k]) for k in ("entry", "nl", "n", "grad", "kind", "sw", "mods") if k in r) + ("-" + r["variant"] if "variant" in r else "")


ROWS = _rows()
_module_cache = {}


def _mods(nl, kind="same"):
    """Three projectors (cached: the rows only flip ``requires_grad``).  ``kind`` breaks the module set in the middle one."""
    import vfa_amd
    if (nl, kind) not in _module_cache:
        def make(channel=256, layers=nl, image_size=(720, 1280)):
            args = SimpleNamespace(data="MultiviewC", image_size=image_size)
            return vfa_amd.VFA(channel, grid_height=32 * layers, cube_size=(25, 25, 32), args=args)
        middle = dict(same={}, c128=dict(channel=128), layers=dict(layers=6 - nl), image_size=dict(image_size=(1080, 1920)))[kind]
        _module_cache[(nl, kind)] = [make(), make(**middle), make()]
    return _module_cache[(nl, kind)]


def _inputs(r, frames=1):
    """mods, maps (laterals or integral images), calibs, grid of a row; gradients wanted as the row says."""
    mods = _mods(r["nl"], r["mods"])
    for m in mods:
        m.collapse.weight.requires_grad_(r["grad"] == "weights")
        m.collapse.bias.requires_grad_(r["grad"] == "weights")
    n = r["n"] * frames
    if r["kind"] == "integrals":
        maps = [torch.zeros(n, 6, 6, m.channel) for m in mods]
    else:
        maps = [torch.zeros(n, m.channel, 4, 4) for m in mods]
    maps[0].requires_grad_(r["grad"] == "lateral")
    calibs = torch.zeros(r["n"], 3, 4, requires_grad=r["grad"] == "calibs")
    return mods, maps, calibs, torch.zeros(1, L, W, 3)


def _install_spies(monkeypatch):
    """The drivers record their name and return zeros of the right shape; the switches are the defaults whatever the environment says."""
    from vfa_amd import lazy, ops, vfa_op
    calls = []

    def frame_spy(name):
        def spy(mods, features, calibs, grid, crange=(-1, 0.95), out=None, **kwargs):
            calls.append(name)
            return out if out is not None else torch.zeros(grid.shape[-3] * grid.shape[-2], 256)
        return spy

    def pipe_frames(mods, features, calibs, grid, n_frames, crange=(-1, 0.95), **kwargs):
        calls.append("pipe_frames")
        return torch.zeros(n_frames, grid.shape[-3] * grid.shape[-2], 256)

    def project_sum(self, features, calibs, grid, crange=(-1, 0.95), out=None, accumulate=False, reserved_cus=0):
        calls.append("project_sum")
        return out if out is not None else torch.zeros(grid.reshape(-1, 3).shape[0], self.collapse.out_features)

    def project_views(self, features, calibs, grid, crange=(-1, 0.95), reserved_cus=0):
        calls.append("project_views")
        return torch.zeros(features.shape[0], grid.reshape(-1, 3).shape[0], self.collapse.out_features)

    for name in ("pipe_frame", "fused_frame", "window_frame", "fused_frame_train"):
        monkeypatch.setattr(vfa_op, name, frame_spy(name))
    monkeypatch.setattr(vfa_op, "pipe_frames", pipe_frames)
    monkeypatch.setattr(vfa_op.VFA, "project_sum", project_sum)
    monkeypatch.setattr(vfa_op.VFA, "project_views", project_views)
    # (the epilogue kernels behind ``project_views``: they have no CPU form either)
    monkeypatch.setattr(ops, "scale_view_sum", lambda lin8, *rest: torch.zeros(lin8.shape[1:]))
    monkeypatch.setattr(ops, "bias_relu_accumulate", lambda lin, bias: torch.zeros(lin.shape[1:]))
    monkeypatch.setattr(lazy, "LAZY", False)
    for name, value in DEFAULTS.items():
        monkeypatch.setattr(vfa_op, name, value)
    return calls


@pytest.fixture
def spies(monkeypatch):
    return _install_spies(monkeypatch)


def _set_switches(monkeypatch, sw):
    from vfa_amd import vfa_op
    for name, value in SWITCHES[sw].items():
        monkeypatch.setattr(vfa_op, name, value)


def _terms(r, mods, maps, calibs):
    """``VFA.forward`` records in the reference's order: cameras outside, scales inside; ``other_cameras``: the middle scale saw
    calibration tensors of its own."""
    from vfa_amd import lazy
    cams = [calibs[c].clone() for c in range(r["n"])]
    others = [c.clone() for c in cams]
    terms = []
    for c in range(r["n"]):
        for k, m in enumerate(mods):
            cal = others[c] if (r["variant"] == "other_cameras" and k == 1) else cams[c]
            feat = maps[k][c:c + 1]
            terms.append((m, feat, lazy.version_of(feat), cal, lazy.version_of(cal)))
    return terms


def _observe(r, calls):
    """Run the row's entry point; what ran: the spies' names in call order ("" = none), or the assertion it raised."""
    import vfa_amd
    from vfa_amd import vfa_op
    del calls[:]
    frames = 2 if r["entry"] == "frames" else 1
    mods, maps, calibs, grid = _inputs(r, frames)
    integrals = maps if r["kind"] == "integrals" else None
    lats = (None, None, None) if integrals is not None else maps
    try:
        with torch.set_grad_enabled(r["grad"] != "off"):
            if r["entry"] == "aggregate":
                out = vfa_amd.aggregate_views(*mods, *lats, calibs, grid, integrals=integrals)
                assert tuple(out.shape) == (1, 256, L, W)
            elif r["entry"] == "frames":
                if r["variant"] == "rig_per_frame":
                    calibs = torch.zeros(2, r["n"], 3, 4)
                out = vfa_amd.aggregate_views(*mods, *lats, calibs, grid, integrals=integrals, frames=2)
                assert tuple(out.shape) == (2, 256, L, W)
            elif r["entry"] == "forward":
                out = mods[0](maps[0], calibs[0], grid)
                assert tuple(out.shape) == (1, 256, L, W)
            else:
                out = vfa_op._materialize(_terms(r, mods, maps, calibs), grid, (-1, 0.95))
                assert tuple(out.shape) == (1, 256, L, W)
    except AssertionError as e:
        return f"AssertionError: {e}"
    return ",".join(calls)


# ------------------------------------------------------------------ part A: the entry points against the recorded parent
def test_the_rows_are_the_recorded_ones():
    golden = json.load(open(GOLDEN_FILE))
    assert sorted(golden) == sorted(_row_id(r) for r in ROWS) and len(golden) == len(ROWS)


@pytest.mark.parametrize("sw", list(SWITCHES))
def test_entry_points_run_the_recorded_drivers(sw, spies, monkeypatch):
    golden = json.load(open(GOLDEN_FILE))
    _set_switches(monkeypatch, sw)
    wrong = {}
    for r in (r for r in ROWS if r["sw"] == sw):
        seen = _observe(r, spies)
        if seen != golden[_row_id(r)]:
            wrong[_row_id(r)] = (seen, golden[_row_id(r)])
    assert not wrong, f"(observed, recorded) of {len(wrong)} rows: {wrong}"


def test_anchor_rows_under_the_default_switches():
    """The rows one can read off the code by hand, as the recorded file has them."""
    golden = json.load(open(GOLDEN_FILE))

    def seen(nl, n, grad, kind="laterals"):
        return golden[_row_id(dict(entry="aggregate", nl=nl, n=n, grad=grad, kind=kind, sw="default", mods="same"))]

    assert seen(1, 7, "off") == DRIVERS["fused"] and seen(1, 7, "weights") == DRIVERS["train"]
    assert seen(5, 7, "off") == DRIVERS["pipe"] and seen(5, 7, "weights") == DRIVERS["train"]
    assert seen(1, 33, "off") == DRIVERS["scale_mfma"] and seen(1, 33, "weights") == DRIVERS["scale_autograd"]
    assert all(seen(5, 33, g) == DRIVERS["scale_autograd"] for g in GRADS)
    assert all(seen(nl, 0, g) == DRIVERS["zeros"] for nl in (1, 5) for g in GRADS)
    assert all(seen(nl, n, "off", "integrals") == "AssertionError: integral-image inputs need a per-frame path" for nl in (1, 5) for n in (0, 33))
    vox = {sw: golden[_row_id(dict(entry="aggregate", nl=1, n=7, grad="off", kind="laterals", sw=sw, mods="same"))] for sw in SWITCHES}
    assert vox["fused_pool_off"] == vox["vox_fits"] == DRIVERS["window"] and vox["vox_too_small"] == DRIVERS["scale_mfma"]


# ------------------------------------------------------------------ part B: frame_route names what part A observed
def _route(*args, **kwargs):
    from vfa_amd import vfa_op
    try:
        return vfa_op.frame_route(*args, **kwargs)
    except AssertionError as e:
        return f"AssertionError: {e}"


def _predicted(r):
    """What the recorded column must hold for this row if ``frame_route`` tells the truth."""
    frames = 2 if r["entry"] == "frames" else 1
    mods, maps, calibs, grid = _inputs(r, frames)
    from_integrals = r["kind"] == "integrals"
    with torch.set_grad_enabled(r["grad"] != "off"):
        if r["entry"] == "aggregate":
            route = _route(mods, r["n"], maps, (calibs, grid), from_integrals=from_integrals)
            return DRIVERS.get(route, route)
        if r["entry"] == "frames":
            # (as the entry point asks: the geometry always, the maps only when they are laterals)
            batch = _route(mods, r["n"], () if from_integrals else maps, (calibs, grid), from_integrals=from_integrals, frames=2)
            if r["variant"] != "rig_per_frame" and batch == "pipe_batch":
                return DRIVERS["pipe_batch"]
            route = _route(mods, r["n"], [m[:r["n"]] for m in maps], (calibs, grid), from_integrals=from_integrals)
            return ",".join([DRIVERS[route]] * 2) if route in DRIVERS else route
        if r["entry"] == "forward":  # one module, one camera: everything between "train" and "scale_autograd" is inside project_sum
            route = _route(mods[:1], 1, maps[:1], (calibs[0], grid))
            return {"train": "fused_frame_train", "scale_autograd": "project_views"}.get(route, "project_sum")
        with torch.no_grad():
            route = _route(mods, r["n"], maps)
        if r["variant"] == "same_cameras" and route in ("pipe", "fused"):
            return DRIVERS[route]
        return ",".join(["project_sum"] * len(mods))


@pytest.mark.parametrize("sw", list(SWITCHES))
def test_frame_route_names_the_recorded_driver(sw, monkeypatch):
    from vfa_amd import vfa_op
    golden = json.load(open(GOLDEN_FILE))
    for name, value in {**DEFAULTS, **SWITCHES[sw]}.items():
        monkeypatch.setattr(vfa_op, name, value)
    wrong = {}
    for r in (r for r in ROWS if r["sw"] == sw):
        if _predicted(r) != golden[_row_id(r)]:
            wrong[_row_id(r)] = (_predicted(r), golden[_row_id(r)])
    assert not wrong, f"(frame_route, recorded) of {len(wrong)} rows: {wrong}"


def test_frame_route_is_pure_and_reads_the_switches_when_called(monkeypatch):
    from vfa_amd import vfa_op
    for name, value in DEFAULTS.items():
        monkeypatch.setattr(vfa_op, name, value)
    r = dict(nl=1, n=7, grad="off", kind="laterals", mods="same")
    mods, maps, calibs, grid = _inputs(r)
    with torch.no_grad():
        assert vfa_op.frame_route(mods, 7, maps, (calibs, grid)) == "fused"
        monkeypatch.setattr(vfa_op, "FUSED_POOL", False)
        assert vfa_op.frame_route(mods, 7, maps, (calibs, grid)) == "window"
        monkeypatch.setattr(vfa_op, "PIPE_SINGLE_LAYER", True)
        assert vfa_op.frame_route(mods, 7, maps, (calibs, grid)) == "pipe"
        assert vfa_op.frame_route(mods, 7, maps, (calibs, grid), frames=2) == "pipe_batch"
        assert mods[0]._defer_ok()
        monkeypatch.setattr(vfa_op, "COLLAPSE_KERNEL", "library")  # (the memo of _defer_ok follows the switches)
        assert vfa_op.frame_route(mods, 7, maps, (calibs, grid)) == "scale_autograd" and not mods[0]._defer_ok()


if __name__ == "__main__":  # record the observations of the code this runs on
    with pytest.MonkeyPatch.context() as mp:
        calls = _install_spies(mp)
        recorded = {}
        for sw in SWITCHES:
            with pytest.MonkeyPatch.context() as inner:
                _set_switches(inner, sw)
                recorded.update({_row_id(r): _observe(r, calls) for r in ROWS if r["sw"] == sw})
    with open(GOLDEN_FILE, "w") as f:
        json.dump(recorded, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(recorded)} rows -> {GOLDEN_FILE}")
