#!/usr/bin/env python3
"""Generate ``iou3d_pairs.npz`` and ``ap_aos_mc.npz`` by RUNNING THE REFERENCE's AP/AOS metric on the CPU.

Runs only where a checkout of the reference is available; ``VFA_REFERENCE_ROOT`` names it.  Nothing of the reference
is copied: the script imports ``vfa.evaluation.pyeval.IoU`` and ``vfa.evaluation.pyeval.evaluateAPAOS`` and calls their own
``IoU3D`` / ``IoUs2D`` / ``cal_frame_TPFP_iou`` / ``CLEAR_MOD_HUN2`` / ``evaluateDetectionAPAOS`` with three stand-ins, all written
here:
  * the extension module ``sort_vertices`` (CUDA-only, cannot be built without nvcc) -> ``oracle/eval_oracle.sort_vertices``,
    the restatement that ``iou_pairs.npz`` pins (the technique of ``make_golden.py:main_iou``);
  * empty ``shapely`` / ``shapely.geometry`` modules (imported at evaluateAPAOS.py:4-5, never used);
  * the ``torch`` name of ``evaluateAPAOS`` replaced by a proxy whose ``device('cuda')`` is the CPU (:79, :82 hard-code it).
Float64 truths of the pair fixture come from an independent polygon clipper (Sutherland-Hodgman + shoelace) times the exact z
overlap.  The script ASSERTS the margins the tests rely on (see ``check_*``); a seed that misses one is not used.

Usage:  VFA_REFERENCE_ROOT=<reference checkout> python tests/golden/make_ap_aos.py      (writes the two files next to this script)
"""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
if not os.environ.get("VFA_REFERENCE_ROOT"):
    raise SystemExit("set VFA_REFERENCE_ROOT to a checkout of the reference")
sys.path.insert(0, os.environ["VFA_REFERENCE_ROOT"])

import torch  # noqa: E402

from oracle import eval_oracle  # noqa: E402

torch.set_num_threads(1)

# --- stand-ins -------------------------------------------------------------------------------------------------------------------
_stub = types.ModuleType("sort_vertices")
_stub.sort_vertices_forward = lambda v, m, nv: torch.from_numpy(eval_oracle.sort_vertices(v.numpy(), m.numpy(), nv.numpy()))
sys.modules["sort_vertices"] = _stub
_shapely, _geometry = types.ModuleType("shapely"), types.ModuleType("shapely.geometry")
_geometry.Polygon = _geometry.MultiPoint = None
_shapely.geometry = _geometry
sys.modules.update({"shapely": _shapely, "shapely.geometry": _geometry})

from vfa.evaluation.pyeval import IoU as ref_iou  # noqa: E402  (the reference)
from vfa.evaluation.pyeval import evaluateAPAOS as ref_eval  # noqa: E402


class _TorchOnCpu:
    """``torch`` as evaluateAPAOS.py sees it: everything is the real module's, except that every device is the CPU."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def device(*_a, **_k):
        return torch.device("cpu")


ref_eval.torch = _TorchOnCpu()

THRESHOLDS = (0.75, 0.5, 0.25)


# --- float64 truth ---------------------------------------------------------------------------------------------------------------
def _corners64(box):
    """Corners of a footprint x y l w alpha in float64, anticlockwise; shares nothing with the reference's corner code."""
    x, y, l, w, a = (float(v) for v in box)
    c, s = np.cos(a), np.sin(a)
    return [(x + dx * l * c - dy * w * s, y + dx * l * s + dy * w * c) for dx, dy in ((.5, .5), (-.5, .5), (-.5, -.5), (.5, -.5))]


def _clip_area(c1, c2):
    """Overlap of two convex quadrilaterals: Sutherland-Hodgman clipping + shoelace in float64."""
    def ccw(poly):
        a = sum(poly[i][0] * poly[(i + 1) % len(poly)][1] - poly[i][1] * poly[(i + 1) % len(poly)][0] for i in range(len(poly)))
        return poly if a > 0 else poly[::-1]
    subject, clip = ccw(list(c1)), ccw(list(c2))
    for i in range(len(clip)):
        a, b = clip[i], clip[(i + 1) % len(clip)]

        def side(p):
            return (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0])
        out = []
        for j in range(len(subject)):
            p, q = subject[j], subject[(j + 1) % len(subject)]
            sp, sq = side(p), side(q)
            if sp >= 0:
                out.append(p)
            if (sp > 0 and sq < 0) or (sp < 0 and sq > 0):
                t = sp / (sp - sq)
                out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
        subject = out
        if not subject:
            return 0.0
    return abs(sum(subject[i][0] * subject[(i + 1) % len(subject)][1] - subject[i][1] * subject[(i + 1) % len(subject)][0]
                   for i in range(len(subject)))) / 2


def truth(b1, b2):
    """(overlap area, BEV IoU, z overlap, 3D IoU) of two fp32 boxes x y z l w h alpha, in float64; z overlap not clamped."""
    b1, b2 = np.asarray(b1, np.float64), np.asarray(b2, np.float64)
    ov = _clip_area(_corners64(b1[[0, 1, 3, 4, 6]]), _corners64(b2[[0, 1, 3, 4, 6]]))
    a1, a2 = b1[3] * b1[4], b2[3] * b2[4]
    zo = min(b1[2] + b1[5] / 2, b2[2] + b2[5] / 2) - max(b1[2] - b1[5] / 2, b2[2] - b2[5] / 2)
    inter = ov * zo
    return ov, ov / (a1 + a2 - ov), zo, inter / (a1 * b1[5] + a2 * b2[5] - inter)


def reference_pair(b1, b2):
    """The reference's own fp32 IoU3D and BEV IoU (and its overlap area) of one pair, the only batch it can run (IoU.py:27-28)."""
    t1, t2 = torch.from_numpy(np.asarray(b1, np.float32)).view(1, 1, 7), torch.from_numpy(np.asarray(b2, np.float32)).view(1, 1, 7)
    with np.errstate(all="ignore"):
        vol = ref_iou.IoU3D(t1, t2)
        bev, _, _, union = ref_iou.IoUs2D(t1[..., [0, 1, 3, 4, 6]], t2[..., [0, 1, 3, 4, 6]])
    return np.float32(vol.item()), np.float32(bev.item()), float(bev.item()) * float(union.item())


# --- fixture 1: box pairs --------------------------------------------------------------------------------------------------------
def main_pairs(seed=71):
    rng = np.random.default_rng(seed)
    u = rng.uniform

    def footprint():
        return [u(-1, 1), u(-1, 1), u(0.5, 3), u(0.5, 3), u(-np.pi, np.pi)]

    def lift(f, z, h):
        return [f[0], f[1], z, f[2], f[3], h, f[4]]

    def random():
        return lift(footprint(), u(-.3, .3), u(.5, 2)), lift(footprint(), u(-.3, .3), u(.5, 2))

    def identical():
        b = lift([u(-1, 1), u(-1, 1), u(.5, 3), u(.5, 3), u(.1, 1.4)], u(-.3, .3), u(.5, 2))
        return b, list(b)

    def contained():
        b = lift([u(-1, 1), u(-1, 1), u(2, 3), u(2, 3), u(.1, 1.4)], 0.0, 2.0)
        return b, lift([b[0] + .1, b[1] - .1, .6, .5, u(-np.pi, np.pi)], u(-.2, .2), 1.0)

    def disjoint():
        f = [u(-1, 1), u(-1, 1), u(.5, 1), u(.5, 1), u(-np.pi, np.pi)]
        return lift(f, u(-.3, .3), u(.5, 2)), lift([f[0] + 5, f[1] + 5, 1, 1, u(-np.pi, np.pi)], u(-.3, .3), u(.5, 2))

    def cows_cm():
        f = [u(500, 3400), u(500, 3400), u(180, 260), u(60, 110), u(-np.pi, np.pi)]
        g = [f[0] + u(-60, 60), f[1] + u(-60, 60), u(180, 260), u(60, 110), f[4] + u(-.5, .5)]
        h1, h2 = u(120, 160), u(120, 160)
        return lift(f, h1 / 2, h1), lift(g, h2 / 2 + u(-10, 10), h2)

    def near(f):
        return [f[0] + u(-.4, .4), f[1] + u(-.4, .4), u(.5, 3), u(.5, 3), u(-np.pi, np.pi)]

    def z_equal():
        f, z, h = footprint(), u(-.3, .3), u(.5, 2)
        return lift(f, z, h), lift(near(f), z, h)

    def z_partial():
        f, h1, h2 = footprint(), u(.5, 2), u(.5, 2)
        return lift(f, 0.0, h1), lift(near(f), u(.2, .8) * (h1 + h2) / 2, h2)

    def z_apart():  # footprints overlap, the boxes do not: the reference's IoU goes negative
        f, h1, h2 = footprint(), u(.5, 2), u(.5, 2)
        return lift(f, 0.0, h1), lift(near(f), (h1 + h2) / 2 + u(.05, 1.5), h2)

    def axis_aligned():  # alpha = 0 / pi/2: parallel edges, zero denominators in the edge-edge intersections
        f = [u(-1, 1), u(-1, 1), u(.5, 3), u(.5, 3), rng.choice([0.0, np.pi / 2])]
        g = [f[0] + u(-.7, .7), f[1] + u(-.7, .7), u(.5, 3), u(.5, 3), rng.choice([0.0, np.pi / 2])]
        return lift(f, u(-.3, .3), u(.5, 2)), lift(g, u(-.3, .3), u(.5, 2))

    plan = [(random, 96), (identical, 12), (contained, 12), (disjoint, 12), (cows_cm, 24), (z_equal, 12), (z_partial, 12),
            (z_apart, 12), (axis_aligned, 24)]
    rows, replaced = [], 0
    for make, count in plan:
        kept = 0
        while kept < count:
            b1, b2 = (np.asarray(b, np.float32) for b in make())
            ov, bev, zo, vol = truth(b1, b2)
            r_vol, r_bev, r_ov = reference_pair(b1, b2)
            area = max(float(b1[3]) * float(b1[4]), float(b2[3]) * float(b2[4]))
            # the project's bound on the reference pipeline (tests/test_eval_ops.py::_check_overlaps), and what follows from it for
            # the ratios; a pair on which the REFERENCE misses it is replaced
            ok = abs(r_ov - ov) <= 1e-4 * area and abs(float(r_bev) - bev) <= 1e-4 and (zo <= 0 or abs(float(r_vol) - vol) <= 1e-4)
            ok = ok and np.isfinite(r_vol) and np.isfinite(r_bev)
            if make is z_apart:
                ok = ok and zo < 0 and ov > 1e-2 and r_vol < 0
            if make is disjoint:
                ok = ok and r_bev == 0 and r_vol == 0
            if not ok:
                replaced += 1
                continue
            rows.append((make.__name__, b1, b2, r_vol, r_bev, ov, bev, zo, vol))
            kept += 1
    kinds = np.array([r[0] for r in rows])
    out = dict(kind=kinds, box1=np.stack([r[1] for r in rows]), box2=np.stack([r[2] for r in rows]),
               ref_iou3d=np.array([r[3] for r in rows], np.float32), ref_iou_bev=np.array([r[4] for r in rows], np.float32),
               overlap=np.array([r[5] for r in rows]), iou_bev=np.array([r[6] for r in rows]),
               z_overlap=np.array([r[7] for r in rows]), iou3d=np.array([r[8] for r in rows]))
    np.savez_compressed(os.path.join(HERE, "iou3d_pairs.npz"), **out)
    for kind in dict.fromkeys(kinds.tolist()):
        sel = kinds == kind
        print(f"iou3d_pairs {kind:13s}: {sel.sum():3d} pairs, reference vs float64: BEV {np.abs(out['ref_iou_bev'] - out['iou_bev'])[sel].max():.1e}"
              f", 3D {np.abs(out['ref_iou3d'] - out['iou3d'])[sel].max():.1e}, 3D IoU {out['iou3d'][sel].min():+.3f} .. {out['iou3d'][sel].max():+.3f}")
    print(f"iou3d_pairs: {len(rows)} pairs, {replaced} candidates replaced")


# --- fixture 2: a MultiviewC-like evaluation set ---------------------------------------------------------------------------------
def synthetic_set(seed):
    """gt rows ``frame x y z l w h rot``, det rows ``frame x y z l w h rot conf``: cow-sized boxes in centimetres on a 39 m field."""
    rng = np.random.default_rng(seed)
    u = rng.uniform
    gt_frames = [2, 5, 6, 11, 14, 20, 27]      # 11: ground truth, no detection
    det_only = [19, 31]                        # 19: detections, no ground truth (false positives); 31: after the last one (dropped)
    gt, det = [], []
    noise = [(4, .02, .03), (12, .05, .08), (25, .10, .2), (45, .15, .45), (90, .2, .9)]  # position cm, relative size, angle
    for f in sorted(gt_frames + det_only):
        cows = []
        if f in gt_frames:
            for _ in range(int(rng.integers(7, 12))):
                h = u(120, 160)
                if cows and u() < 0.3:  # a neighbour lying against the previous cow: detections with a second candidate
                    c = cows[-1]
                    cows.append([c[0] + u(-70, 70), c[1] + u(-70, 70), h / 2, u(180, 260), u(60, 110), h, c[6] + u(-.4, .4)])
                else:
                    cows.append([u(300, 3600), u(300, 3600), h / 2, u(180, 260), u(60, 110), h, u(-np.pi, np.pi)])
            gt += [[f] + c for c in cows]
        if f == 11:
            continue
        for c in cows:
            if u() < 0.12:
                continue  # missed
            pos, rel, ang = noise[int(rng.choice(5, p=[.3, .25, .2, .15, .1]))]
            d = [c[0] + rng.normal(0, pos), c[1] + rng.normal(0, pos), c[2] + rng.normal(0, pos / 4), c[3] * (1 + rng.normal(0, rel)),
                 c[4] * (1 + rng.normal(0, rel)), c[5] * (1 + rng.normal(0, rel)), c[6] + rng.normal(0, ang)]
            det.append([f] + d + [u(.4, 1.0) - pos / 300])
            if u() < 0.15:  # a second, worse detection of the same cow: several detections may match one ground truth
                det.append([f] + [d[0] + rng.normal(0, 20), d[1] + rng.normal(0, 20)] + d[2:] + [u(.3, .6)])
        for _ in range(int(rng.integers(2, 5))):
            h = u(120, 160)
            det.append([f, u(300, 3600), u(300, 3600), h / 2, u(180, 260), u(60, 110), h, u(-np.pi, np.pi), u(.3, .7)])
    gt, det = np.round(np.array(gt, np.float64), 4), np.round(np.array(det, np.float64), 4)
    det[:, 8] = np.round(det[:, 8], 6)
    return gt, det


def run_reference(gt, det):
    """The reference's evaluateDetectionAPAOS on the two arrays written as text files, with its per-pair IoUs and per-frame match
    tables recorded on the way (wrappers around its own IoU3D and cal_frame_TPFP_iou; nothing is replaced)."""
    ious, tables = [], {t: [] for t in THRESHOLDS}
    orig_iou, orig_frame = ref_eval.IoU3D, ref_eval.cal_frame_TPFP_iou

    def iou3d(a, b):
        out = orig_iou(a, b)
        ious.append((np.float32(out.item()), a.numpy().reshape(7).copy(), b.numpy().reshape(7).copy()))
        return out

    def frame(thresh, gt_res, pred_res):
        out = orig_frame(thresh, gt_res, pred_res)
        tables[thresh].append((int(pred_res.shape[0]), int(gt_res.shape[0]), out.copy()))
        return out
    ref_eval.IoU3D, ref_eval.cal_frame_TPFP_iou = iou3d, frame
    try:
        with tempfile.TemporaryDirectory() as tmp, np.errstate(all="ignore"):
            np.savetxt(os.path.join(tmp, "gt.txt"), gt)
            np.savetxt(os.path.join(tmp, "det.txt"), det)
            nine = ref_eval.evaluateDetectionAPAOS(os.path.join(tmp, "det.txt"), os.path.join(tmp, "gt.txt"))
    finally:
        ref_eval.IoU3D, ref_eval.cal_frame_TPFP_iou = orig_iou, orig_frame
    return np.array(nine, np.float64), ious, tables


def check_margins(iou, det_begin, gt_begin, pair_begin, rows, conf):
    """The conditions that keep the tests from resting on rounding; returns the smallest margins for the log."""
    to_thresh = min(float(np.abs(iou - t).min()) for t in THRESHOLDS)
    assert to_thresh >= 1e-3, f"an IoU within {to_thresh:.1e} of a threshold"
    gap = np.inf
    for f in range(len(det_begin) - 1):
        P, G = det_begin[f + 1] - det_begin[f], gt_begin[f + 1] - gt_begin[f]
        if P == 0 or G < 2:
            continue
        m = np.sort(iou[pair_begin[f]:pair_begin[f + 1]].reshape(P, G), axis=1)
        contested = m[:, -2] >= 0.2
        if contested.any():
            gap = min(gap, float((m[:, -1] - m[:, -2])[contested].min()))
    assert gap >= 1e-3, f"best and second-best IoU of a detection {gap:.1e} apart"
    assert len(np.unique(conf)) == len(conf), "equal confidences"
    for t in THRESHOLDS:
        matched = rows[t][:, 1] >= 0
        assert not (rows[t][matched][:, [0, 3]] == -1.0).any(), "an exact -1.0 in a matched row"
        assert np.array_equal(rows[t][:, 4] == 1, matched)
    return to_thresh, gap


def main_set(seeds=range(81, 200)):
    for seed in seeds:
        gt, det = synthetic_set(seed)
        nine, ious, tables = run_reference(gt, det)
        # the three passes see the same pairs in the same order; the first one's IoUs are the record
        n = len(ious) // 3
        assert len(ious) == 3 * n and all(np.array_equal(ious[k][0], ious[k + n][0]) for k in range(n))
        iou = np.array([v for v, _, _ in ious[:n]], np.float32)
        frames_t = tables[THRESHOLDS[0]]
        det_begin = np.concatenate([[0], np.cumsum([p for p, _, _ in frames_t])]).astype(np.int32)
        gt_begin = np.concatenate([[0], np.cumsum([g for _, g, _ in frames_t])]).astype(np.int32)
        pair_begin = np.concatenate([[0], np.cumsum([p * g for p, g, _ in frames_t])]).astype(np.int64)
        assert pair_begin[-1] == n
        rows = {t: np.concatenate([r for _, _, r in tables[t]], axis=0) for t in THRESHOLDS}
        try:
            to_thresh, gap = check_margins(iou, det_begin, gt_begin, pair_begin, rows, det[:, 8])
        except AssertionError as e:
            print(f"ap_aos_mc: seed {seed} not used: {e}")
            continue
        # the boxes as the reference hands them to IoU3D (float64 text values -> fp32), in its frame-counter order
        det_frames = np.unique(det[:, 0])
        walked = det_frames[:len(frames_t)]
        det_boxes = np.concatenate([det[det[:, 0] == f, 1:8] for f in walked]).astype(np.float32)
        gt_boxes = np.concatenate([gt[gt[:, 0] == f, 1:8] for f in walked]).astype(np.float32)
        assert len(det_boxes) == det_begin[-1] and len(gt_boxes) == gt_begin[-1]
        for f in range(len(frames_t)):
            G = gt_begin[f + 1] - gt_begin[f]
            for k in range(pair_begin[f], pair_begin[f + 1]):
                i, j = divmod(k - pair_begin[f], G)
                assert np.array_equal(det_boxes[det_begin[f] + i], ious[k][1]) and np.array_equal(gt_boxes[gt_begin[f] + j], ious[k][2])
        kept = np.isin(gt[:, 0], np.unique(det[:, 0]))
        assert kept.sum() == gt_begin[-1] and (~kept).any() and det_begin[-1] < len(det)
        assert any(p > 0 and g == 0 for p, g, _ in frames_t), "no frame with detections and without ground truth"
        np.savez_compressed(os.path.join(HERE, "ap_aos_mc.npz"), gt=gt, det=det, seed=np.array(seed), thresholds=np.array(THRESHOLDS),
                            nine=nine, iou=iou, det_begin=det_begin, gt_begin=gt_begin, pair_begin=pair_begin, n_gt=np.array(kept.sum()),
                            det_boxes=det_boxes, gt_boxes=gt_boxes, rows_75=rows[0.75], rows_50=rows[0.5], rows_25=rows[0.25])
        print(f"ap_aos_mc: seed {seed}: {len(gt)} ground truths ({kept.sum()} counted), {len(det)} detections ({det_begin[-1]} walked), "
              f"{len(frames_t)} frame counters, {n} pairs; nearest IoU to a threshold {to_thresh:.1e}, best - second {gap:.1e}")
        print("ap_aos_mc: AP / AOS / OS at 0.75, 0.5, 0.25:", np.round(nine, 4).tolist())
        print("ap_aos_mc: matched at 0.75 / 0.5 / 0.25:", [int((rows[t][:, 4] == 1).sum()) for t in THRESHOLDS])
        return
    raise SystemExit("no seed met the margins")


if __name__ == "__main__":
    if "--pairs" in sys.argv:
        main_pairs()
    elif "--set" in sys.argv:
        main_set()
    else:
        main_pairs()
        main_set()
