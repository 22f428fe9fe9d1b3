"""SimOTA matching + ComputeLoss.ota_loss: the device kernels vs the reference-run golden
(tests/golden/ota.npz, made by `python -m oracle.make_golden ota`) and vs the oracle restatement on other seeds."""
import types

import numpy as np
import pytest
import torch

from oracle import losses as o_loss
from tests.conftest import golden


def _inputs(seed=7, B=2, nc=6, shapes=((80, 80), (40, 40), (20, 20)), n_per=(3, 12)):
    """same generator as oracle/make_golden.py::ota_inputs (the golden stores the targets, not the logits)"""
    rng = np.random.default_rng(seed)
    rows = []
    for b in range(B):
        n = int(rng.integers(*n_per))
        xy = rng.uniform(0.02, 0.98, (n, 2))
        wh = np.exp(rng.uniform(np.log(0.02), np.log(0.7), (n, 2)))
        cls = rng.integers(0, 80, (n, 1))
        rows.append(np.concatenate((np.full((n, 1), b), cls, xy, wh), 1))
    t = np.concatenate(rows, 0).astype(np.float32)
    t[0, 2:4] = [0.999, 0.0005]
    t[-1, 2:4] = [0.5, 0.5]
    t[:, 1] = rng.integers(0, nc, t.shape[0])
    p = [rng.normal(0, 1.5, (B, 3, ny, nx, 5 + nc)).astype(np.float32) for ny, nx in shapes]
    for pi in p:
        pi[..., :4] *= 0.3
    return t, p


def _cfg(nc):
    import os
    from efficientteacher_amd.configs import get_cfg
    from tests.conftest import ROOT
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "efficientteacher_amd/configs/ssod/coco-standard/yolov5l_coco_ssod_10_percent.yaml"))
    cfg.merge_from_list(["Dataset.nc", nc, "Loss.assigner_type", "SimOTA"])
    return cfg


def _closs(anchors, nc, dev):
    from efficientteacher_amd.models.loss import ComputeLoss
    head = types.SimpleNamespace(nl=3, na=3, nc=nc, num_keypoints=0, anchors=torch.as_tensor(anchors).to(dev),
                                 stride=torch.tensor([8., 16., 32.]))
    return ComputeLoss(types.SimpleNamespace(head=head), _cfg(nc))


def _match_lists(match, table, nl, na):
    """device match array -> per level (slot, target row) in slot order"""
    NT = table.shape[0]
    m = match.cpu().numpy().reshape(nl, 5 * na * NT)
    out = []
    for i in range(nl):
        slots = np.nonzero(m[i] >= 0)[0]
        out.append((slots, m[i][slots]))
    return out


def test_golden_matching_and_loss(hip):
    from efficientteacher_amd import ops
    g = golden("ota")
    nc = int(g["nc"])
    t, p_np = _inputs(nc=nc)
    assert np.array_equal(t, g["targets"])
    closs = _closs(g["anchors"], nc, hip.device)
    assert closs.ota and np.allclose([closs.box_w, closs.obj_w, closs.cls_w, closs.anchor_t], g["weights"])
    p = [hip.t(x).requires_grad_(True) for x in p_np]
    # --- matching: (b, a, gj, gi, target row) per level, bit-exact, in reference order within an image --------------------
    tt = hip.t(t)
    table = torch.cat((tt, torch.zeros((t.shape[0], 1), device=hip.device), torch.ones((t.shape[0], 1), device=hip.device)), 1)
    match = ops.ota_assign([x.detach() for x in p], table, closs._anchors_host, closs._strides, nc=nc,
                           anchor_t=float(closs.anchor_t), top_k=closs.top_k)
    lists = _match_lists(match, table, 3, 3)
    for i in range(3):
        slots, rows = lists[i]
        ref_rows = g[f"l{i}_target"]
        ref_slot = g[f"l{i}_slot"]            # index into the level's candidate list (reference order)
        assert len(slots) == ref_rows.shape[0], (i, len(slots), ref_rows.shape[0])
        # device slots are numbered over ALL (offset, anchor, target) combinations, the reference's over the surviving
        # candidates; both orders are offset-major / anchor / target, so sorting by slot and by candidate index must agree
        # once the reference rows are regrouped from image-major to slot order
        order = np.argsort(ref_slot, kind="stable")
        assert np.array_equal(t[rows], ref_rows[order]), i
    # --- loss, items, gradients ---------------------------------------------------------------------------------------------
    loss, items = closs(p, tt)
    ref = float(g["loss"][0])
    assert abs(loss.item() - ref) <= 1e-4 * abs(ref), (loss.item(), ref)
    assert np.allclose([items[k].item() for k in ("box", "obj", "cls")], g["items"], rtol=1e-4, atol=1e-6)
    loss.backward()
    g2 = g["grad2"]
    assert np.abs(p[2].grad.cpu().numpy() - g2).max() <= 1e-4 * np.abs(g2).max() + 1e-7
    for i in range(2):
        gr = p[i].grad.cpu()
        b, a, gj, gi = (torch.from_numpy(g[f"l{i}_{k}"]) for k in ("b", "a", "gj", "gi"))
        rows = gr[b, a, gj, gi].numpy()
        refr = g[f"gradrows{i}"]
        assert np.abs(rows - refr).max() <= 1e-4 * np.abs(refr).max() + 1e-7, i
        sums = gr.double().sum((0, 1, 2, 3)).numpy()
        assert np.allclose(sums, g[f"gradsum{i}"], rtol=1e-3, atol=1e-5), i


@pytest.mark.parametrize("seed,B,n_per,dtype", [(1, 3, (1, 6), torch.float32), (2, 2, (20, 40), torch.float32),
                                                 (3, 4, (0, 3), torch.float32), (4, 2, (5, 9), torch.bfloat16)])
def test_vs_oracle(hip, seed, B, n_per, dtype):
    """other seeds / crowded images (many multiply-claimed candidates) / images without targets / bf16 logits"""
    nc = 6
    g = golden("ota")
    shapes = ((40, 40), (20, 20), (10, 10)) if hip.emulated else ((80, 80), (40, 40), (20, 20))
    rng = np.random.default_rng(100 + seed)
    rows = []
    for b in range(B):
        n = int(rng.integers(n_per[0], n_per[1] + 1))
        if seed == 3 and b == 1:
            n = 0
        xy = rng.uniform(0.02, 0.98, (n, 2))
        wh = np.exp(rng.uniform(np.log(0.03), np.log(0.5), (n, 2)))
        rows.append(np.concatenate((np.full((n, 1), b), rng.integers(0, nc, (n, 1)), xy, wh), 1))
    t = np.concatenate(rows, 0).astype(np.float32)
    t = t[rng.permutation(t.shape[0])]                  # targets need not arrive grouped by image
    p_np = [rng.normal(0, 1.0, (B, 3, ny, nx, 5 + nc)).astype(np.float32) for ny, nx in shapes]
    for pi in p_np:
        pi[..., :4] *= 0.3
    closs = _closs(g["anchors"], nc, hip.device)
    # the oracle scales gt boxes by the reference's literal 640; on the emulator's 320-pixel pyramid that only shifts the IoUs
    if dtype == torch.bfloat16:
        p_np = [torch.from_numpy(x).to(torch.bfloat16).float().numpy() for x in p_np]
    p = [hip.t(x, dtype).requires_grad_(True) for x in p_np]
    loss, items = closs(p, hip.t(t))
    loss.backward()
    po = [torch.from_numpy(x).requires_grad_(True) for x in p_np]
    lo, io = o_loss.ota_loss(po, torch.from_numpy(t), torch.from_numpy(g["anchors"]), closs._strides, nc=nc, box_w=closs.box_w,
                             obj_w=closs.obj_w, cls_w=closs.cls_w, anchor_t=closs.anchor_t)
    lo.backward()
    # the bf16 logits are pre-rounded and the kernel's arithmetic is fp32 in every mode: the values meet the fp32 bound, and the
    # gradient is rounded once to bf16 (unit roundoff 2^-8), per element, on top of the fp32 kernel-vs-oracle term
    # (tests/test_lp_logits.py::test_simota_head_views holds the same inputs to these bounds on strided head views, fp16 included)
    assert abs(loss.item() - lo.item()) <= 1e-4 * abs(lo.item()), (loss.item(), lo.item())
    for k in ("box", "obj", "cls"):
        assert abs(items[k].item() - io[k].item()) <= 1e-4 * abs(io[k].item()) + 1e-6, k
    for a, b in zip(p, po):
        ref = b.grad.numpy()
        err = np.abs(a.grad.float().cpu().numpy() - ref)
        if dtype == torch.float32:
            assert err.max() <= 1e-4 * np.abs(ref).max() + 1e-7, err.max()
        else:
            assert (err <= 2.0 ** -8 * np.abs(ref) + 2e-4 * np.abs(ref).max()).all(), (err.max(), np.abs(ref).max())


def test_padding_rows_and_empty(hip):
    """rows with flags 0 (the fixed-capacity table of the captured step) take no part; no targets at all -> default empty loss"""
    from efficientteacher_amd import ops
    g = golden("ota")
    nc = int(g["nc"])
    t, p_np = _inputs(nc=nc)
    closs = _closs(g["anchors"], nc, hip.device)
    p = [hip.t(x) for x in p_np]
    tt = hip.t(t)
    n = t.shape[0]
    table = torch.cat((tt, torch.zeros((n, 1), device=hip.device), torch.ones((n, 1), device=hip.device)), 1)
    pad = torch.zeros((5, 8), device=hip.device)
    pad[:, 2:6] = 0.5
    padded = torch.cat((table[:3], pad[:2], table[3:], pad[2:]), 0)
    l1, _ = closs.ota_loss(p, None, table=table)
    l2, _ = closs.ota_loss(p, None, table=padded)
    assert abs(l1.item() - l2.item()) <= 1e-6 * abs(l1.item())
    l0, _ = closs(p, torch.zeros((0, 6), device=hip.device))
    ref0, _ = o_loss.ota_loss([torch.from_numpy(x) for x in p_np], torch.zeros((0, 6)), torch.from_numpy(g["anchors"]),
                              closs._strides, nc=nc, box_w=closs.box_w, obj_w=closs.obj_w, cls_w=closs.cls_w,
                              anchor_t=closs.anchor_t)
    assert abs(l0.item() - ref0.item()) <= 1e-4 * abs(ref0.item())


def test_oracle_reproduces_reference_golden():
    """the restatement (oracle/losses.py build_ota_targets / ota_loss) against what the reference produced"""
    g = golden("ota")
    nc = int(g["nc"])
    t, p_np = _inputs(nc=nc)
    anchors = torch.from_numpy(g["anchors"])
    strides = [float(s) for s in g["strides"]]
    po = [torch.from_numpy(x).requires_grad_(True) for x in p_np]
    res = o_loss.build_ota_targets([x.detach() for x in po], torch.from_numpy(t), anchors, strides, nc=nc, anchor_t=float(g["weights"][3]))
    for i in range(3):
        for k in ("b", "a", "gj", "gi", "slot"):
            assert np.array_equal(res[i][k].numpy(), g[f"l{i}_{k}"]), (i, k)
        assert np.array_equal(res[i]["target"].numpy(), g[f"l{i}_target"])
    w = g["weights"]
    loss, items = o_loss.ota_loss(po, torch.from_numpy(t), anchors, strides, nc=nc, box_w=w[0], obj_w=w[1], cls_w=w[2], anchor_t=w[3])
    loss.backward()
    assert np.allclose(loss.detach().numpy(), g["loss"], rtol=1e-6)
    assert np.allclose(po[2].grad.numpy(), g["grad2"], rtol=1e-5, atol=1e-8)
