"""What tests/test_decode_fused_cpu.py and tests/test_decode_fused.py share: a numpy restatement of the decode half of the reference's
``ObjectEncoder`` (vfa/data/encoder.py:234-305) in the form the fused call promises -- candidates ``conf > thresh``, the first ``k`` by
confidence descending and cell ascending (a stable arg-sort), fp32 box arithmetic -- and the decoders / heads of the fixtures."""
import numpy as np

from conftest import golden_path

FIXTURES = ("decode_mc.npz", "decode_wt.npz", "decode_mx.npz")
THRESH = 0.4  # the threshold the fixtures were recorded at (tests/test_eval_ops.py)
F = np.float32


def sigmoid32(x):
    """``1.0f / (1.0f + expf(-x))`` in float32 (numpy's exp for the device's expf: equal within a few ulps)."""
    with np.errstate(over="ignore"):
        return (F(1) / (F(1) + np.exp(-np.asarray(x, F)))).astype(F)


def restate(conf_map, loc, thresh, topk, grid_size, world_size, yx_first=False, dim=None, rot=None, mean=None):
    """One frame.  ``conf_map (L, W)``: the NMS output; ``loc (L, W, 2)``; in 3D ``dim (L, W, 3)``, ``rot (L, W, R)``, ``mean (3)``.
    -> dict of ``cell (n)``, ``conf (n)``, ``location (n, 3)`` and in 3D ``dimension (n, 3)``, ``rotation (n)``, ``rot_index (n)``."""
    L, W = conf_map.shape
    flat = np.asarray(conf_map, F).ravel()
    k = min(topk, L * W)
    order = np.argsort(-flat, kind="stable")[:k]               # confidence descending, equal ones by ascending cell
    cell = order[flat[order] > F(thresh)]
    l, w = cell // W, cell % W
    t = np.asarray(loc, F)[l, w]
    cy = ((l.astype(F) + sigmoid32(t[:, 0])) / F(grid_size[0]) * F(world_size[0])).astype(F)
    cx = ((w.astype(F) + sigmoid32(t[:, 1])) / F(grid_size[1]) * F(world_size[1])).astype(F)
    first, second = (cy, cx) if yx_first else (cx, cy)
    out = {"cell": cell.astype(np.int32), "conf": flat[cell], "location": np.stack([first, second, np.zeros_like(cx)], axis=-1)}
    if rot is not None:
        d = np.asarray(dim, F)[l, w]
        out["dimension"] = (np.exp(d) * np.asarray(mean, F)[None, :]).astype(F)
        out["rot_index"] = np.argmax(sigmoid32(np.asarray(rot, F)[l, w]), axis=-1)   # (numpy: the first index of the maximum)
        out["rotation"] = (out["rot_index"].astype(F) * F(0.017453292519943295)).astype(F)
    return out


def load(name):
    d = np.load(golden_path(name))
    return d, str(d["base"]) == "MultiviewC"


def decoder_of(d, topk=100, with_mean=True):
    from vfa_amd import eval_ops
    return eval_ops.BEVDecoder(str(d["base"]), tuple(d["world_size"]), tuple(d["cube_LWH"]),
                               dimension_mean=d["dimension_mean"] if with_mean else None, topk=topk)


def restate_fixture(d, conf_map=None, thresh=THRESH, topk=100):
    three_d = str(d["base"]) == "MultiviewC"
    grid_size = np.asarray(d["world_size"], np.float64) / np.asarray(d["cube_LWH"], np.float64)[:2]
    return restate(d["nms"][0, 0] if conf_map is None else conf_map, d["loc_offset"][0], thresh, topk, grid_size, d["world_size"],
                   yx_first=str(d["base"]) == "Wildtrack", dim=d["dim_offset"][0] if three_d else None,
                   rot=d["rotation_logits"][0] if three_d else None, mean=d["dimension_mean"] if three_d else None)


def by_conf_x_y(conf, loc):
    """The ordering tests/test_eval_ops.py compares the decode under: equal confidences come out of ``topk`` in no particular order."""
    return np.lexsort((np.round(loc[:, 1], 3), np.round(loc[:, 0], 3), -conf))
