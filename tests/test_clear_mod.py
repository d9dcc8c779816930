"""The CLEAR-MOD metric (MODA / MODP) on the MI355X (-m gpu): the one-wave-per-frame distance + Hungarian assignment kernel
(``vfa_clear_mod_frames_f64``) against numpy's float64 distances, scipy's per-frame records and the reference's recorded numbers
(tests/golden/clear_mod.npz, generated from the reference by tests/golden/make_clear_mod.py).

Bounds, derivations and not measurements: distances are compared BITWISE (float64 subtract, multiply, add and a correctly rounded
square root in the reference's order).  A frame's cost sum is a float64 sum of at most 130 terms no larger than 30, added in another
order than scipy's record: the rounding error is near 1e-14 relative, 1e-9 is the project's margin for such sums
(tests/test_ap_aos_cpu.py).  The four metrics are quotients of exact integers and of one such sum: 1e-9 relative as well."""
import itertools

import numpy as np
import pytest
import torch

from conftest import golden_path

pytestmark = pytest.mark.gpu

TD = 30.0
SETS = ("demo1", "demo2", "syn")


def _dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fixture():
    return np.load(golden_path("clear_mod.npz"))


def _frames_of(d, name):
    """The set as sorted rows + frame counters over the frames the records describe."""
    gt, det, ids = d[f"{name}_gt"], d[f"{name}_det"], d[f"{name}_frame_ids"]
    gt, det = gt[np.isin(gt[:, 0], ids)], det[np.isin(det[:, 0], ids)]
    gt_ctr, det_ctr = np.searchsorted(ids, gt[:, 0]), np.searchsorted(ids, det[:, 0])
    go, do = np.argsort(gt_ctr, kind="stable"), np.argsort(det_ctr, kind="stable")
    return gt[go, 1:3], gt_ctr[go], det[do, 1:3], det_ctr[do], len(ids)


@pytest.fixture(scope="module")
def tables(fixture):
    """One launch per set, with the matrices; shared by the tests below and left unchanged."""
    from vfa_amd import eval_ops
    out = {}
    for name in SETS:
        gt_xy, gt_ctr, det_xy, det_ctr, n_frames = _frames_of(fixture, name)
        t = eval_ops.match_frames_hungarian(torch.from_numpy(det_xy).to(_dev()), torch.from_numpy(det_ctr).to(_dev()),
                                            torch.from_numpy(gt_xy).to(_dev()), torch.from_numpy(gt_ctr).to(_dev()),
                                            n_frames=n_frames, td=TD, with_matrix=True)
        out[name] = (gt_xy, gt_ctr, det_xy, det_ctr, n_frames, type(t)(*[None if v is None else v.cpu().numpy() for v in t]))
    return out


def _numpy_distances(g_xy, d_xy):
    dx, dy = g_xy[:, None, 0] - d_xy[None, :, 0], g_xy[:, None, 1] - d_xy[None, :, 1]
    return np.sqrt(dx * dx + dy * dy)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("name", SETS)
def test_distance_matrices_are_numpys_bits(tables, name):
    gt_xy, gt_ctr, det_xy, det_ctr, n_frames, t = tables[name]
    assert t.pair_begin[0] == 0 and t.pair_begin[-1] == len(t.dist)
    worst = 0
    for f in range(n_frames):
        want = _numpy_distances(gt_xy[gt_ctr == f], det_xy[det_ctr == f])
        got = t.dist[t.pair_begin[f]:t.pair_begin[f + 1]].reshape(want.shape)
        worst = max(worst, int(np.abs(_bits(got) - _bits(want)).max(initial=0)))
    print(f"{name}: largest difference of a distance from numpy's, in units of the last place: {worst}")
    assert worst == 0


def test_distances_next_to_the_threshold_are_numpys_bits(fixture):
    """One ground truth, detections whose dx^2 + dy^2 lies within a few ulps of td^2 on both sides: the square root's bits, and the
    strict comparison with td that follows from them."""
    from vfa_amd import eval_ops
    g_xy, d_xy = fixture["near_td_gt"], fixture["near_td_det"]
    want = _numpy_distances(g_xy, d_xy)[0]
    assert (want < TD).any() and (want >= TD).any()
    n = len(d_xy)  # each detection alone with the ground truth, as the frames of one launch
    t = eval_ops.match_frames_hungarian(torch.from_numpy(d_xy).to(_dev()), torch.arange(n, device=_dev()),
                                        torch.from_numpy(np.repeat(g_xy, n, axis=0)).to(_dev()), torch.arange(n, device=_dev()),
                                        n_frames=n, td=TD, with_matrix=True)
    got = t.dist.cpu().numpy()
    print("ulps from numpy:", (_bits(got) - _bits(want)).tolist())
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(t.gt_match.cpu().numpy(), np.where(want < TD, 0, -1))
    assert np.array_equal(t.frame_counts.cpu().numpy()[:, 2], (want < TD).astype(np.int64))


@pytest.mark.parametrize("name", SETS)
def test_frame_tables_against_scipy_records(fixture, tables, name):
    gt_xy, gt_ctr, det_xy, det_ctr, n_frames, t = tables[name]
    records, cost_sum = fixture[f"{name}_records"], fixture[f"{name}_cost_sum"]
    unique, tied, want_match = fixture[f"{name}_unique"], fixture[f"{name}_tied"], fixture[f"{name}_gt_match"]
    assert (t.frame_status == 0).all()
    assert np.array_equal(t.frame_counts[:, :3], records[:, :3].astype(np.int64))  # g, n_det, c: exact
    rel = np.abs(t.frame_cost - cost_sum) / np.maximum(cost_sum, 1e-300)
    print(f"{name}: largest relative difference of a frame's cost sum from scipy's record {rel[cost_sum > 0].max(initial=0):.2e}")
    assert (np.abs(t.frame_cost - cost_sum) <= 1e-9 * cost_sum).all()
    compared = 0
    for f in range(n_frames):
        rows = np.flatnonzero(gt_ctr == f)
        P = int((det_ctr == f).sum())
        match, dist = t.gt_match[rows], t.gt_dist[rows]
        matrix = t.dist[t.pair_begin[f]:t.pair_begin[f + 1]].reshape(len(rows), P)
        hit = match >= 0
        assert ((match >= -1) & (match < max(P, 1))).all() and len(np.unique(match[hit])) == hit.sum() == records[f, 2]  # one-to-one
        assert (dist[hit] < TD).all() and np.array_equal(_bits(dist[hit]), _bits(matrix[np.flatnonzero(hit), match[hit]]))
        assert np.isposinf(dist[~hit]).all()
        assert abs(dist[hit].sum() - records[f, 3]) <= 1e-9 * records[f, 3]
        # pairs assigned at 1e6, at exactly td (cost sum - matched sum) and matched make up the smaller side
        at_td = round((t.frame_cost[f] - dist[hit].sum()) / TD)
        assert hit.sum() + at_td + t.frame_counts[f, 3] == min(len(rows), P)
        if unique[f] and not tied[f]:
            assert np.array_equal(match, want_match[rows]), f"frame {f}"
            compared += 1
    assert compared >= n_frames - 1


def test_named_frames(fixture, tables):
    gt_xy, gt_ctr, det_xy, det_ctr, n_frames, t = tables["syn"]
    records, counts = fixture["syn_records"], t.frame_counts
    sizes = [(int(g), int(p)) for g, p in records[:, :2]]
    # the frame of integer coordinates with pairs at exactly td: the reference's c, and a pair at td assigned without being a match
    at_td = [f for f in range(n_frames) if sizes[f][0] and sizes[f][1] and (gt_xy[gt_ctr == f] % 1 == 0).all() and (det_xy[det_ctr == f] % 1 == 0).all()]
    assert len(at_td) == 1
    f = at_td[0]
    matched = t.gt_dist[gt_ctr == f]
    assert counts[f, 2] == records[f, 2] and t.frame_cost[f] - matched[np.isfinite(matched)].sum() >= TD
    # every pair beyond td
    beyond = [f for f in range(n_frames) if sizes[f][0] and sizes[f][1] and records[f, 2] == 0]
    assert len(beyond) == 1
    f = beyond[0]
    assert counts[f, 2] == 0 and counts[f, 3] == min(sizes[f]) and t.frame_cost[f] == 0 and (t.gt_match[gt_ctr == f] == -1).all()
    for f in range(n_frames):  # empty sides
        if 0 in sizes[f]:
            assert counts[f].tolist() == [sizes[f][0], sizes[f][1], 0, 0] and t.frame_cost[f] == 0 and t.frame_status[f] == 0


def test_empty_frames_touch_no_neighbours_rows(fixture):
    """The entry point itself on sentinel-filled outputs: frames without ground truth, without detections or without both write
    their counts and nothing into the tables around them; rows outside the frames keep their sentinels."""
    from vfa_amd import _lib
    dev = _dev()
    rng = np.random.default_rng(5)
    sizes = [(3, 4), (0, 0), (0, 5), (2, 2), (5, 0), (0, 0), (1, 3)]  # (G, P)
    gt_begin, det_begin = np.cumsum([0] + [g for g, _ in sizes]) + 2, np.cumsum([0] + [p for _, p in sizes]) + 1  # rows in front too
    n_gt, n_det = int(gt_begin[-1]) + 3, int(det_begin[-1]) + 2                                                       # ... and behind
    gt_xy, det_xy = rng.uniform(0, 40, (n_gt, 2)), rng.uniform(0, 40, (n_det, 2))
    to = lambda a, dt: torch.from_numpy(np.asarray(a)).to(dev, dt)
    gt_match = torch.full((n_gt,), -77, dtype=torch.int32, device=dev)
    gt_dist = torch.full((n_gt,), -77.0, dtype=torch.float64, device=dev)
    counts = torch.full((len(sizes), 4), -77, dtype=torch.int64, device=dev)
    cost = torch.full((len(sizes),), -77.0, dtype=torch.float64, device=dev)
    status = torch.full((len(sizes),), -77, dtype=torch.int32, device=dev)
    g, d = to(gt_xy, torch.float64), to(det_xy, torch.float64)
    gb, db = to(gt_begin, torch.int32), to(det_begin, torch.int32)
    _lib.call("vfa_clear_mod_frames_f64", _lib.ptr(d), _lib.ptr(db), _lib.ptr(g), _lib.ptr(gb), len(sizes), n_det, n_gt, TD, None, 0, None,
              _lib.ptr(gt_match), _lib.ptr(gt_dist), _lib.ptr(counts), _lib.ptr(cost), _lib.ptr(status), _lib.current_stream_handle())
    gt_match, gt_dist, counts, cost, status = (v.cpu().numpy() for v in (gt_match, gt_dist, counts, cost, status))
    assert (status == 0).all() and np.array_equal(counts[:, :2], np.array(sizes))
    inside = np.zeros(n_gt, bool)
    inside[gt_begin[0]:gt_begin[-1]] = True
    assert (gt_match[~inside] == -77).all() and (gt_dist[~inside] == -77.0).all()
    assert (gt_match[inside] != -77).all() and (gt_dist[inside] != -77.0).all()
    for f, (G, P) in enumerate(sizes):
        dist = _numpy_distances(gt_xy[gt_begin[f]:gt_begin[f + 1]], det_xy[det_begin[f]:det_begin[f + 1]])
        c = np.where(dist > TD, 1e6, dist)
        c = c if G <= P else c.T  # the best of all injections of the smaller side, by brute force (at most 4 x 3 x 2 of them)
        best = min((tuple(c[i, k] for i, k in enumerate(cols)) for cols in itertools.permutations(range(c.shape[1]), c.shape[0])), key=sum)
        assert counts[f, 2] == sum(v < TD for v in best) and counts[f, 3] == sum(v == 1e6 for v in best)
        assert abs(cost[f] - sum(v for v in best if v < 1e6)) <= 1e-9 * max(cost[f], 1.0)
        if G == 0 or P == 0:
            assert cost[f] == 0 and counts[f, 2] == 0 and (gt_match[gt_begin[f]:gt_begin[f + 1]] == -1).all()


def test_a_frame_over_the_cap_is_refused_in_place():
    """513 detections in the middle frame: status 1, -1 / +inf in its rows, its counts untouched, the neighbours solved."""
    from vfa_amd import eval_ops
    dev = _dev()
    cap = eval_ops.CLEAR_MOD_MAX_SIDE
    det_xy = torch.cat([torch.tensor([[1.0, 1.0]]), torch.arange(2.0 * (cap + 1)).reshape(-1, 2), torch.tensor([[5.0, 5.0]])]).to(dev)
    det_frame = torch.tensor([0] + [1] * (cap + 1) + [2], device=dev)
    gt_xy = torch.tensor([[1.0, 2.0], [0.0, 0.0], [3.0, 3.0], [5.0, 9.0]], device=dev)
    gt_frame = torch.tensor([0, 1, 1, 2], device=dev)
    t = eval_ops.match_frames_hungarian(det_xy, det_frame, gt_xy, gt_frame, n_frames=3)
    assert t.frame_status.tolist() == [0, 1, 0]
    assert t.gt_match.tolist() == [0, -1, -1, 0] and t.gt_dist.tolist() == [1.0, float("inf"), float("inf"), 4.0]
    assert t.frame_counts.tolist() == [[1, 1, 1, 0], [0, 0, 0, 0], [1, 1, 1, 0]]


def test_no_synchronisation_when_n_frames_is_given(tables):
    from vfa_amd import eval_ops
    gt_xy, gt_ctr, det_xy, det_ctr, n_frames, want = tables["syn"]
    args = [torch.from_numpy(a).to(_dev()) for a in (det_xy, det_ctr, gt_xy, gt_ctr)]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        t = eval_ops.match_frames_hungarian(*args, n_frames=n_frames, td=TD)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert np.array_equal(t.gt_match.cpu().numpy(), want.gt_match) and t.dist is None
    again = eval_ops.match_frames_hungarian(*args)  # n_frames from the counters: the same tables
    assert torch.equal(again.gt_match, t.gt_match) and torch.equal(again.frame_counts, t.frame_counts)
    with pytest.raises(ValueError):
        eval_ops.match_frames_hungarian(args[0], args[1].flip(0), args[2], args[3])


@pytest.mark.parametrize("name", SETS)
def test_clear_mod_meets_the_reference(fixture, tmp_path, name):
    from vfa_amd import eval_ops
    gt, det, four = fixture[f"{name}_gt"], fixture[f"{name}_det"], fixture[f"{name}_four"]
    got = eval_ops.clear_mod(gt, det)
    for label, mine, ref in zip(("recall", "precision", "MODA", "MODP"), got, four):
        print(f"{name} {label}: {mine:.14f} (reference {ref:.14f}, relative difference {abs(mine - ref) / ref:.2e})")
    assert all(abs(mine - ref) <= 1e-9 * abs(ref) for mine, ref in zip(got, four))
    c, fp, m, g, _ = eval_ops.clear_mod_totals(gt, det)
    assert [c, fp, m, g] == fixture[f"{name}_totals"].tolist()  # exact
    res, gtf = str(tmp_path / "res.txt"), str(tmp_path / "gt.txt")
    np.savetxt(res, det, "%.17g")
    np.savetxt(gtf, gt, "%.17g")
    assert eval_ops.evaluate_detection(res, gtf, "Wildtrack") == got == eval_ops.evaluate_detection(res, gtf)
    shuffled = np.random.default_rng(3).permutation(len(gt))  # rows of the frames interleaved: the set is sorted inside
    got_shuffled = eval_ops.clear_mod(gt[shuffled], det[::-1])
    assert got_shuffled[:3] == got[:3] and abs(got_shuffled[3] - got[3]) <= 1e-9 * got[3]


def test_two_runs_give_identical_bits(tables):
    from vfa_amd import eval_ops
    for name in SETS:
        gt_xy, gt_ctr, det_xy, det_ctr, n_frames, first = tables[name]
        args = [torch.from_numpy(a).to(_dev()) for a in (det_xy, det_ctr, gt_xy, gt_ctr)]
        second = eval_ops.match_frames_hungarian(*args, n_frames=n_frames, td=TD, with_matrix=True)
        for a, b in zip(first, second):
            b = b.cpu().numpy()
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
