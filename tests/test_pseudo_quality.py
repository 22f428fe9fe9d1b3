"""Pseudo-label hit rate on the device (csrc/pseudo_quality.hip: et_pseudo_quality; ops.pseudo_label_quality;
utils/self_supervised_utils.py: pseudo_label_hit_rate, check_pseudo_label_with_gt; the trainers' statistic).

* the numpy helper tests/pseudo_quality_ref.py is pinned on tests/golden/pseudo_quality.npz, which tools/make_pseudo_quality_golden.py
  made from the live reference (check_pseudo_label_with_gt, check_pseudo_label);
* the kernels against the golden on cases A (mixed), B (wide), C (crowded), D0 / D1 / D2 (degenerate), with and without ground
  truth: EQUALITY of all five fp64 values -- the counts are integers and each rate is one IEEE fp64 division of the same two integers on
  both sides.
"""
import inspect
import sys
import types

import numpy as np
import pytest
import torch

from tests import pseudo_quality_ref as pr
from tests.conftest import golden

MODES = {True: "with_gt", False: "without_gt"}


def _case(name):
    g = golden("pseudo_quality")
    c = {k: g[f"{name}_{k}"] for k in ("t9", "valid", "gt", "lo", "hi", "with_gt", "without_gt")}
    c["bs"] = int(g[f"{name}_bs"])
    return c


def _operands(hip, c):
    return (hip.t(c["t9"]), hip.t(c["valid"]), hip.t(c["gt"]), hip.t(c["lo"]), hip.t(c["hi"]), c["bs"])


def _same(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    print("got ", got.tolist(), "\nwant", want.tolist())
    return got.shape == want.shape and got.tobytes() == (want + 0.0).tobytes()        # + 0.0: no negative zero in a golden


# ---- the helper is the reference ---------------------------------------------------------------------------------------
def test_helper_equals_golden():
    for name in pr.CASES:
        c = _case(name)
        assert c["t9"].shape == (c["bs"] * pr.MAX_DET, 9) and c["t9"].dtype == np.float64 and c["gt"].dtype == np.float32
        assert np.array_equal(c["t9"], c["t9"].astype(np.float32).astype(np.float64))     # the table holds fp32 numbers
        for with_gt, key in MODES.items():
            assert _same(pr.hit_rate(c["t9"], c["valid"], c["gt"], c["lo"], c["hi"], c["bs"], with_gt), c[key]), (name, key)
    # case A holds what it is there for: every category counts, and "distinct labels" is not "rows"
    a = _case("A")
    rel, unc = pr.split_rows(a["t9"], a["valid"], a["lo"], a["hi"])
    iou, cats = pr.categories(a["t9"][unc].astype(np.float32), a["gt"])
    counts = [pr.distinct_labels(iou, q) for q in cats]
    assert min(n for n, _ in counts) >= 3 and any(n < len(picked) for n, picked in counts)
    v, cls = a["valid"].astype(bool), a["t9"][:, 1].astype(int)
    on_hi, on_lo = v & (a["t9"][:, 6] == a["hi"][cls]), v & (a["t9"][:, 6] == a["lo"][cls])
    assert (on_hi & rel).any() and not (on_hi & unc).any() and (on_lo & unc).any()       # the >= / < sides
    assert rel.any() and (v & ~rel & ~unc).any() and (~v & (a["t9"][:, 6] > 0)).any()    # reliable, below low, poisoned padding
    b, c = _case("B"), _case("C")
    assert b["bs"] == 32 and c["bs"] == 2 and (c["gt"][:, 0] == 0).sum() == 150
    assert _case("D0")["gt"].shape == (0, 6) and not _case("D1")["valid"].any() and _case("D2")["valid"].any()


# ---- the op against the golden ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_gt", [True, False])
@pytest.mark.parametrize("name", pr.CASES)
def test_op_equals_golden(hip, name, with_gt):
    from efficientteacher_amd import ops
    c = _case(name)
    t9, valid, gt, lo, hi, bs = _operands(hip, c)
    gt0 = gt.clone()
    out = ops.pseudo_label_quality(t9, valid, gt, lo, hi, bs, with_gt=with_gt)
    assert out.shape == (5,) and out.dtype == torch.float64 and out.device.type == hip.device.type
    assert _same(out.tolist(), c[MODES[with_gt]])
    assert torch.equal(gt, gt0)                                                          # the reference scales it in place; not here
    assert _same(out.tolist(), pr.hit_rate(c["t9"], c["valid"], c["gt"], c["lo"], c["hi"], bs, with_gt))
    again = ops.pseudo_label_quality(t9, valid, gt, lo, hi, bs, with_gt=with_gt)
    assert torch.equal(out, again)


def test_hit_rate_dict(hip):
    from efficientteacher_amd.utils.self_supervised_utils import pseudo_label_hit_rate
    c = _case("A")
    for with_gt, key in MODES.items():
        d = pseudo_label_hit_rate(*_operands(hip, c), with_gt)
        assert list(d) == ["tp", "fp_cls", "fp_loc", "pse_num", "gt_num"]
        assert all(v.dim() == 0 and v.dtype == torch.float64 and v.device.type == hip.device.type for v in d.values())
        assert _same(torch.stack(list(d.values())).tolist(), c[key])


def test_reference_signature(hip):
    from efficientteacher_amd.utils.self_supervised_utils import check_pseudo_label_with_gt
    c = _case("A")
    rows = hip.t(c["t9"][c["valid"].astype(bool)])
    labels = hip.t(c["gt"])
    keep = labels.clone()
    got = check_pseudo_label_with_gt(rows, labels, ignore_thres_low=c["lo"].tolist(), ignore_thres_high=c["hi"].tolist(), batch_size=c["bs"])
    assert len(got) == 5 and all(isinstance(r, np.ndarray) and r.shape == (1,) for r in got[:3])
    assert _same([float(r[0]) for r in got[:3]] + [got[3], got[4]], c["with_gt"])
    assert torch.equal(labels, keep)
    got = check_pseudo_label_with_gt(rows.float(), labels, iouv=torch.tensor([0.5]), ignore_thres_low=c["lo"].tolist(),
                                     ignore_thres_high=c["hi"].tolist(), batch_size=c["bs"])   # an fp32 table holds the same numbers
    assert _same([float(r[0]) for r in got[:3]] + [got[3], got[4]], c["with_gt"])
    with pytest.raises(NotImplementedError):
        check_pseudo_label_with_gt(rows, labels, iouv=torch.linspace(0.5, 0.95, 10), ignore_thres_low=c["lo"].tolist(),
                                   ignore_thres_high=c["hi"].tolist())
    # no uncertain row: integer zeros for the rates, as the reference gives them (D2); no row at all: gt_num is still M / bs
    d = _case("D2")
    got = check_pseudo_label_with_gt(hip.t(d["t9"][d["valid"].astype(bool)]), hip.t(d["gt"]), ignore_thres_low=d["lo"].tolist(),
                                     ignore_thres_high=d["hi"].tolist(), batch_size=d["bs"])
    assert got[:3] == (0, 0, 0) and _same([0, 0, 0, got[3], got[4]], d["with_gt"])
    got = check_pseudo_label_with_gt(rows[:0], labels, ignore_thres_low=c["lo"].tolist(), ignore_thres_high=c["hi"].tolist(), batch_size=4)
    assert got == (0, 0, 0, 0.0, labels.shape[0] / 4)
    # without thresholds every row takes part (the reference's else branch): the helper with thresholds nothing falls outside of
    every = pr.hit_rate(c["t9"], c["valid"], c["gt"], [-np.inf], [np.inf], c["bs"])
    got = check_pseudo_label_with_gt(rows, labels, batch_size=c["bs"])
    assert every[3] * c["bs"] == rows.shape[0] and _same([float(r[0]) for r in got[:3]] + [got[3], got[4]], every)


def test_equal_iou_takes_the_lower_label_index(hip):
    """two labels placed symmetrically about pseudo row 0 (every coordinate exact in fp32, so the two IoUs are equal); pseudo row 1
    prefers label 1.  Lower index on the tie: labels {0, 1} are picked, tp = 2 / 2; the other way round it would be 1 / 2."""
    from efficientteacher_amd import ops
    gt = np.array([[0, 2, 0.46875, 0.5, 0.25, 0.25], [0, 2, 0.53125, 0.5, 0.25, 0.25]], np.float32)
    t9 = np.zeros((8, 9), np.float64)
    t9[0] = [0, 2, 0.5, 0.5, 0.25, 0.25, 0.3, 0.3, 0.3]
    t9[5] = [0, 2, 0.546875, 0.5, 0.25, 0.25, 0.3, 0.3, 0.3]
    valid = np.zeros(8, np.uint8)
    valid[[0, 5]] = 1
    lo, hi = np.array([0.1] * 3), np.array([0.6] * 3)
    iou, cats = pr.categories(t9[[0, 5]].astype(np.float32), gt)
    assert iou[0, 0] == iou[1, 0] >= 0.5 and iou[1, 1] > iou[0, 1] >= 0.5
    want = pr.hit_rate(t9, valid, gt, lo, hi, 1)
    assert want.tolist() == [1.0, 0.0, 0.0, 2.0, 2.0]
    out = ops.pseudo_label_quality(hip.t(t9), hip.t(valid), hip.t(gt), hip.t(lo), hip.t(hi), 1)
    assert _same(out.tolist(), want)
    # the labels in the other order: the tie now goes to the label that row 1 prefers as well, one distinct label
    rev = gt[::-1].copy()
    assert pr.hit_rate(t9, valid, rev, lo, hi, 1).tolist() == [0.5, 0.0, 0.0, 2.0, 2.0]
    out = ops.pseudo_label_quality(hip.t(t9), hip.t(valid), hip.t(rev), hip.t(lo), hip.t(hi), 1)
    assert _same(out.tolist(), [0.5, 0.0, 0.0, 2.0, 2.0])


# ---- the trainers' statistic -------------------------------------------------------------------------------------------------
class _Loss:
    def __init__(self, lo, hi):
        from efficientteacher_amd import ops
        self.ignore_thres_low, self.ignore_thres_high, self._thr = list(lo), list(hi), ops.DeviceThresholds()

    def refresh_thresholds(self, dev):
        return self._thr.refresh(self.ignore_thres_low, self.ignore_thres_high, dev)


def _trainer_stub(hip, c, with_gt):
    t9, valid, gt, lo, hi, bs = _operands(hip, c)
    return types.SimpleNamespace(_last_pseudo=(t9, valid), compute_un_sup_loss=_Loss(c["lo"], c["hi"]), batch_size=bs, WORLD_SIZE=1,
                                 target_with_gt=with_gt), gt


def test_adapters_statistic_needs_neither_the_users_tree_nor_the_host(hip, monkeypatch):
    """the adapters' code path with ``utils.self_supervised_utils`` of the user's tree unimportable and ``Tensor.cpu`` raising"""
    from efficientteacher_amd.trainer.adapters import _SsodHotPath
    monkeypatch.setitem(sys.modules, "utils", None)                                      # `import utils...` raises ImportError
    monkeypatch.setitem(sys.modules, "utils.self_supervised_utils", None)
    with pytest.raises(ImportError):
        import utils.self_supervised_utils  # noqa: F401
    c = _case("A")
    stub, gt = _trainer_stub(hip, c, True)

    def no_cpu(self, *a, **k):
        raise AssertionError("Tensor.cpu() called")
    monkeypatch.setattr(torch.Tensor, "cpu", no_cpu)
    d = _SsodHotPath._pseudo_label_hit_rate(stub, gt)
    stub.target_with_gt = False
    d0 = _SsodHotPath._pseudo_label_hit_rate(stub, gt)
    monkeypatch.undo()
    assert _same(torch.stack(list(d.values())).tolist(), c["with_gt"])
    assert _same(torch.stack(list(d0.values())).tolist(), c["without_gt"])


def test_core_trainer_statistic(hip):
    from efficientteacher_amd.trainer.ssod_trainer import SSODTrainer
    c = _case("A")
    stub, gt = _trainer_stub(hip, c, True)
    d = SSODTrainer.pseudo_label_hit_rate(stub, gt)
    assert _same(torch.stack(list(d.values())).tolist(), c["with_gt"])
    d = SSODTrainer.pseudo_label_hit_rate(stub, with_gt=False)
    assert _same(torch.stack(list(d.values())).tolist(), c["without_gt"])
    with pytest.raises(ValueError):
        SSODTrainer.pseudo_label_hit_rate(stub)                                          # with_gt from the recipe, no labels given
    stub._last_pseudo = None
    with pytest.raises(RuntimeError):
        SSODTrainer.pseudo_label_hit_rate(stub, gt)


def test_cpu_tensor_is_refused():
    from efficientteacher_amd import _lib, ops
    _lib._use_library_for_tests(None, False)
    c = _case("D0")
    cpu = [torch.as_tensor(c[k]) for k in ("t9", "valid", "gt", "lo", "hi")]
    for with_gt in (True, False):
        with pytest.raises(_lib.EtHipError):
            ops.pseudo_label_quality(*cpu, c["bs"], with_gt=with_gt)


def test_statistic_has_no_host_transfer_in_its_source():
    """companion of the GPU sync-debug test below"""
    from efficientteacher_amd import ops
    from efficientteacher_amd.trainer.adapters import _SsodHotPath
    from efficientteacher_amd.trainer.ssod_trainer import SSODTrainer
    from efficientteacher_amd.utils import self_supervised_utils as ssu
    for fn in (ops.pseudo_label_quality, ssu.pseudo_label_hit_rate, _SsodHotPath._pseudo_label_hit_rate, SSODTrainer.pseudo_label_hit_rate):
        src = inspect.getsource(fn)
        for word in (".item(", ".cpu(", ".tolist(", ".numpy(", "synchronize", "import utils", "from utils", ".any()", "[v]"):
            assert word not in src, (fn.__name__, word)


@pytest.mark.gpu
def test_hit_rate_does_not_synchronise():
    from efficientteacher_amd import _lib
    from efficientteacher_amd.utils.self_supervised_utils import pseudo_label_hit_rate
    from tests.conftest import _Mode
    _lib._use_library_for_tests(None, False)
    _lib.load()
    hip = _Mode("cuda:0", False)
    c = _case("C")
    args = _operands(hip, c)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):                        # torch must honour the mode here, or the test shows nothing
            args[1].sum().item()
        d1 = pseudo_label_hit_rate(*args, True)
        d0 = pseudo_label_hit_rate(*args, False)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert _same(torch.stack(list(d1.values())).tolist(), c["with_gt"])
    assert _same(torch.stack(list(d0.values())).tolist(), c["without_gt"])
