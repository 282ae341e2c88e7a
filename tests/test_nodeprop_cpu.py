"""CPU checks of node property prediction: the float64 restatement (tests/nodeprop_ref.py) against the golden captured
from the reference's NodePredictor (tests/golden/node_pred.npz) and against sklearn's ndcg_score; the label stream,
its schedule, its CSV reader and the synthetic labels (tgnx/nodeprop.py); the module's construction and state dict."""
import os

import numpy as np
import pytest
import torch

import nodeprop_ref as R

PARAMS = ("lin_node.weight", "lin_node.bias", "out.weight", "out.bias")


def _close(a, b, tol, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(float(np.abs(b).max()), 1.0) if b.size else 1.0
    err = float(np.abs(a - b).max()) if b.size else 0.0
    print(f"{what}: err {err:.3e} scale {scale:.3e}")
    assert err <= tol * scale, (what, err, scale)


def test_ref_reproduces_the_golden(golden):
    """The golden holds float32 results of torch on the CPU: the float64 restatement agrees within float32 rounding of
    100-term dot products (2e-5 forward, 1e-4 gradients: the GPU tests' bounds)."""
    g = golden("node_pred.npz")
    sd = {n: g["sd." + n] for n in PARAMS}
    logits, h = R.head_forward(g["z"], sd["lin_node.weight"], sd["lin_node.bias"], sd["out.weight"], sd["out.bias"])
    _close(logits, g["logits"], 2e-5, "logits")
    loss, dl = R.soft_ce(logits, g["y"])
    _close(loss.mean(), g["loss"], 2e-5, "loss")
    assert loss[5] == 0.0 and not dl[5].any()                      # the all-zero target row
    gr = R.head_backward(dl, g["z"], h, sd["lin_node.weight"], sd["out.weight"])
    for name, key in (("lin_node.weight", "dw1"), ("lin_node.bias", "db1"), ("out.weight", "dw2"), ("out.bias", "db2")):
        _close(gr[key], g["grad." + name], 1e-4, f"d{name}")
    _close(gr["dz"], g["dz"], 1e-4, "dz")


def _ndcg_cases(C, seed):
    """(scores, targets) rows: random, all tied, half tied, rounded scores; the targets random sparse, all zero, all
    one."""
    rng = np.random.default_rng(seed)
    rows = 8
    s = rng.standard_normal((rows, C))
    s[1] = 0.25                                                     # all tied
    s[2, : C // 2] = s[2, 0]                                        # half tied
    s[3] = np.round(s[3], 1)                                        # many small tie groups
    s[4] = np.round(s[4], 0)
    y = rng.random((rows, C)) * (rng.random((rows, C)) < 0.3)
    y[5] = 0.0                                                      # no positive target
    y[6] = 1.0                                                      # all one
    y[1] = np.round(y[1], 1)                                        # tied targets under tied scores
    return s, y


@pytest.mark.parametrize("C", [2, 7, 65, 255, 1001])
@pytest.mark.parametrize("k", [3, 10])
def test_ndcg_rows_equals_sklearn(C, k):
    metrics = pytest.importorskip("sklearn.metrics")
    s, y = _ndcg_cases(C, 100 + C)
    got = R.ndcg_rows(s, y, k)
    for i in range(s.shape[0]):
        want = metrics.ndcg_score(y[i:i + 1], s[i:i + 1], k=k)
        assert abs(got[i] - want) <= 1e-12, (C, k, i, got[i], want)
    assert got[5] == 0.0


def _stream(t, src, dst):
    from types import SimpleNamespace
    return SimpleNamespace(t=np.asarray(t, dtype=np.float64), src=np.asarray(src), dst=np.asarray(dst))


def test_label_stream_coalesces_duplicates_and_groups():
    from tgnx.nodeprop import LabelStream
    #            row 0: classes 3, 1, 3      row 1: none      row 2: 0, 0
    ls = LabelStream([1.0, 1.0, 4.0], [7, 2, 7], [0, 3, 3, 5], [3, 1, 3, 0, 0], [0.25, 0.5, 0.25, 1.0, 2.0], 5)
    assert ls.ptr.tolist() == [0, 2, 2, 3]
    assert ls.cls.tolist() == [1, 3, 0] and ls.w.tolist() == [0.5, 0.5, 3.0]
    T, lo, hi = ls.groups()
    assert T.tolist() == [1.0, 4.0] and lo.tolist() == [0, 2] and hi.tolist() == [2, 3]
    y = ls.dense(0, 3, "cpu")
    assert y.tolist() == [[0, 0.5, 0, 0.5, 0], [0, 0, 0, 0, 0], [3.0, 0, 0, 0, 0]]
    assert ls.dense(1, 3, "cpu").tolist() == y[1:].tolist() and ls.dense(2, 2, "cpu").shape == (0, 5)
    with pytest.raises(ValueError, match="sorted by time"):
        LabelStream([2.0, 1.0], [0, 1], [0, 0, 0], [], [], 3)
    with pytest.raises(ValueError, match="classes"):
        LabelStream([1.0], [0], [0, 1], [3], [1.0], 3)


def test_label_schedule_on_a_hand_made_stream():
    from tgnx.nodeprop import LabelStream, label_schedule
    ev_t = np.array([10.0, 20.0, 20.0, 30.0, 40.0, 50.0])
    #                 before every event | equal to events 1, 2 | between 3 and 4 | after the last
    lt = [5.0, 20.0, 20.0, 35.0, 60.0]
    ls = LabelStream(lt, [0, 1, 2, 3, 4], np.arange(6), [0] * 5, [1.0] * 5, 2)
    full = label_schedule(ev_t, ls, 0, 6)
    # T = 20: the events AT 20 come after the label (r = 1: only the event at 10 is seen); T = 5 is skipped
    assert full == [(1, 1, 3), (4, 3, 4), (6, 4, 5)]
    # adjacent passes partition the groups
    for cut in range(7):
        assert label_schedule(ev_t, ls, 0, cut) + label_schedule(ev_t, ls, cut, 6) == full, cut
    assert label_schedule(ev_t, ls, 1, 4) == [(4, 3, 4)]
    # fp32 event times (the engine's table): the label times are rounded the same way
    big = np.array([1.5e9, 1.5e9 + 1000.0], dtype=np.float32)
    ls2 = LabelStream([1.5e9 + 1.0, 1.5e9 + 1001.0], [0, 1], [0, 1, 2], [0, 1], [1.0, 1.0], 2)
    assert label_schedule(big, ls2, 0, 2) == [(1, 1, 2)]            # 1.5e9 + 1 rounds onto the first event: r = 0


def test_make_labels_rows_sum_to_one():
    from tgnx.nodeprop import make_labels
    from tgnx.synth import make_stream
    s = make_stream("tgbl-wiki", seed=5, num_events=600, num_nodes=60, msg_dim=8)
    C = 7
    period = (s.t[-1] - s.t[0]) / 6
    ls = make_labels(s, C, period)
    y = ls.dense(0, len(ls), "cpu").double().numpy()
    assert len(ls) > 0 and np.abs(y.sum(1) - 1.0).max() < 1e-6 and (y >= 0).all()
    T, lo, hi = ls.groups()
    assert 5 <= T.shape[0] <= 7 and T[0] == s.t[0]
    # row (T_j, u) is the class histogram of u's destinations in (T_j, T_j + period]
    for r in (0, len(ls) // 2, len(ls) - 1):
        m = (s.src == ls.node[r]) & (s.t > ls.t[r]) & (s.t <= ls.t[r] + period)
        want = np.bincount(s.dst[m] % C, minlength=C) / m.sum()
        assert np.abs(y[r] - want).max() < 1e-6, r
    # a node without events in a window has no row there
    g0 = set(ls.node[lo[1]:hi[1]].tolist())
    assert g0 == set(s.src[(s.t > T[1]) & (s.t <= T[1] + period)].tolist())


def test_read_node_labels_csv_round_trip(tmp_path):
    from tgnx.nodeprop import read_node_labels_csv
    from tgnx.tgb_io import read_edgelist_csv
    edge, lab = tmp_path / "e_edgelist.csv", tmp_path / "e_node_labels.csv"
    edge.write_text("ts,src,dst,w\n1,u9,g1,1.0\n2,u3,g2,1.0\n3,u9,g2,2.0\n")
    lab.write_text("ts,node,class,weight\n2,u9,rock,0.75\n2,u9,jazz,0.25\n2,u3,jazz,1.0\n5,u9,rock,0.5\n"
                   "5,u9,rock,0.25\n")
    src, dst, _, _ = read_edgelist_csv(str(edge))
    ls = read_node_labels_csv(str(edge), str(lab))
    assert src.tolist() == [0, 2, 0] and dst.tolist() == [1, 3, 3]   # u9 -> 0, g1 -> 1, u3 -> 2, g2 -> 3
    assert ls.num_classes == 2 and ls.class_keys == ["rock", "jazz"]
    assert ls.t.tolist() == [2.0, 2.0, 5.0] and ls.node.tolist() == [0, 2, 0]
    assert ls.dense(0, 3, "cpu").tolist() == [[0.75, 0.25], [0.0, 1.0], [0.75, 0.0]]
    lab.write_text("ts,node,class,weight\n2,nobody,rock,1.0\n")
    with pytest.raises(ValueError, match="does not occur"):
        read_node_labels_csv(str(edge), str(lab))


def test_node_predictor_module_without_a_gpu(golden):
    from modules.decoder import NodePredictor
    import pyg_epoch_utils
    import tgnx.nn as tnn
    from tgnx import nodeprop, ops
    assert NodePredictor is tnn.NodePredictor and "NodePredictor" in tnn.__all__
    assert pyg_epoch_utils.NodePredictor is tnn.NodePredictor
    assert pyg_epoch_utils.train_node is nodeprop.train_node and pyg_epoch_utils.test_node is nodeprop.test_node
    head = NodePredictor(100, 65)
    assert {k: tuple(v.shape) for k, v in head.state_dict().items()} == {
        "lin_node.weight": (100, 100), "lin_node.bias": (100,), "out.weight": (65, 100), "out.bias": (65,)}
    g = golden("node_pred.npz")
    head.load_state_dict({n: torch.from_numpy(g["sd." + n]) for n in PARAMS}, strict=True)
    assert torch.equal(head.out.bias, torch.from_numpy(g["sd.out.bias"]))
    ns = ops.load()
    for name in ("node_predictor", "node_predictor_bwd", "node_loss_ndcg"):
        assert name in ops.OPS and hasattr(ns, name), name
    assert ops.ndcg_cum(3) == pytest.approx(R.ndcg_cum(3).tolist(), abs=0, rel=1e-15)
    assert os.path.exists(os.path.join(os.path.dirname(__file__), "golden", "make_node_pred_golden.py"))
