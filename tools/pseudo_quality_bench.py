"""Time the pseudo-label hit rate inside the SSOD step, on one GPU in one process.

    python tools/pseudo_quality_bench.py [--per-rank 32] [--steps 50] [--rounds 3] [--out profiles/pseudo_quality_mi355x.txt]

The step is bench.py's v5l-ssod workload (build_trainer / make_batch / synth_teacher_scores imported from it) with synthetic ground
truth of COCO density (about 7 labels per unlabeled image).  Legs, alternated within the process, `rounds` times each:
  (1) the step, no statistic;
  (2) the step + the device statistic with ground truth (SSODTrainer.pseudo_label_hit_rate: launches only);
  (2r) the same + one read of the five numbers, which is what a progress bar does;
  (3) the step + the host path the statistic replaces: boolean-index compaction, .cpu() of table and labels, a per-row python
      selection loop, matching by tests/pseudo_quality_ref.py (the helper, not the code under test; what the reference does);
  (2m) / (3m) legs 2 and 3 once more with the STATISTIC's upper threshold at the median confidence of the step's pseudo labels, so
      that about half of the rows are uncertain and are matched (bench.py's synthetic teacher scores put every row above the
      recipe's threshold, where neither path has anything to match); the step itself keeps the recipe's thresholds;
  (4) the step + the statistic without ground truth as the adapter computed it before the kernel existed (a chain of torch ops);
  (5) the step + the device statistic without ground truth.
Per leg: ms per step over `steps` steps between two device synchronisations (median of the rounds, and the spread), and the
isolated cost of the statistic between two device synchronisations after a step (median of 20).  The device numbers are compared
with the helper's before any time is reported."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (imported, not edited)
from efficientteacher_amd.utils.self_supervised_utils import pseudo_label_hit_rate  # noqa: E402
from tests import pseudo_quality_ref as pr  # noqa: E402
from tools.val_metrics_bench import clocks  # noqa: E402


def synth_gt(rng, B, per_image=7.0):
    rows = []
    for b in range(B):
        n = int(rng.poisson(per_image))
        xy = rng.uniform(0.1, 0.9, (n, 2))
        wh = np.minimum(np.exp(rng.uniform(np.log(0.02), np.log(0.6), (n, 2))), 2 * np.minimum(xy, 1 - xy))
        rows.append(np.concatenate((np.full((n, 1), b), rng.integers(0, 80, (n, 1)), xy, wh), 1))
    return torch.from_numpy(np.concatenate(rows, 0).astype(np.float32))


def host_with_gt(t9, valid, gt, lo, hi, bs):
    """leg 3: what the reference's rank 0 does after every step, with the helper as the matching routine"""
    rows = t9[valid.bool()]                                       # compaction: a host synchronisation
    if rows.shape[0] == 0:
        return np.zeros(5)
    rows_h, gt_h = rows.cpu(), gt.cpu()                           # fp64 rows, as the reference's trainer holds them
    unc = []
    for t in rows_h:                                              # the reference's select_targets: one python iteration per row
        if t[6] >= hi[int(t[1])]:
            continue
        elif t[6] >= lo[int(t[1])]:
            unc.append(np.array(t))
    out = np.zeros(5)
    if unc:
        out[:3] = np.array(pr.match_counts(np.array(unc).astype(np.float32), gt_h.numpy()), np.float64) / len(unc)
    out[3], out[4] = len(unc) / bs, gt_h.shape[0] / bs
    return out


def torch_chain_without_gt(t9, valid, lo_list, hi_list, bs):
    """leg 4: the adapter's statistic without ground truth before the kernel existed"""
    lo = torch.as_tensor(lo_list, dtype=torch.float64, device=t9.device)
    hi = torch.as_tensor(hi_list, dtype=torch.float64, device=t9.device)
    v = valid.bool()
    cls = t9[:, 1].long().clamp_(0, lo.numel() - 1)
    conf = t9[:, 6]
    reliable = (v & (conf >= hi[cls])).sum().double() / bs
    uncertain = (v & (conf < hi[cls]) & (conf >= lo[cls])).sum().double() / bs
    n = v.sum().double()
    both = reliable + uncertain
    zero = torch.zeros((), dtype=torch.float64, device=t9.device)
    tp = torch.where(both > 0, reliable / both.clamp_min(1e-300), zero)
    recall = torch.where(n > 0, both * bs / n.clamp_min(1.0), zero)
    return torch.stack((tp, zero, recall, both, reliable))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--per-rank", type=int, default=32)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    B = a.per_rank
    cfg, tr = bench.build_trainer(dev, 0, 1, 0, B)
    rng = np.random.default_rng(1234)
    S = cfg.Dataset.img_size
    imgs, targets, u_str, u_ori, M_s = bench.make_batch(rng, B, B, S, dev)
    imgs, u_str, u_ori = [(t * 255).round().to(torch.uint8) for t in (imgs, u_str, u_ori)]
    synth = bench.synth_teacher_scores(cfg, B, S, torch.Generator(device="cpu").manual_seed(99)).to(dev)

    def hook(tp):
        tp[..., 4:] = synth
        return tp
    tr.teacher_pred_hook = hook
    gt = synth_gt(rng, B).to(dev)
    loss = tr.compute_un_sup_loss
    lo_list, hi_list = list(loss.ignore_thres_low), list(loss.ignore_thres_high)
    bs = tr.batch_size
    counter = [2000]

    def step():
        counter[0] += 1
        return tr.train_instance(imgs, targets, None, u_str, u_ori, None, M_s, counter[0])

    for _ in range(a.warmup):
        step()
    # thresholds for the legs 2m / 3m: the recipe's lower one, the median confidence of this step's pseudo labels as the upper one
    t9, valid = tr._last_pseudo
    mid = float(t9[valid.bool(), 6].median()) if bool(valid.any()) else hi_list[0]
    hi_mid = [max(mid, lo + 1e-3) for lo in lo_list]
    thr_mid = torch.tensor([lo_list, hi_mid], dtype=torch.float64).to(dev)

    stats = {
        "1  step, no statistic": lambda: None,
        "2  + device statistic, with gt": lambda: tr.pseudo_label_hit_rate(gt, with_gt=True),
        "2r + device statistic, with gt, read": lambda: torch.stack(list(tr.pseudo_label_hit_rate(gt, with_gt=True).values())).tolist(),
        "3  + host path, with gt": lambda: host_with_gt(*tr._last_pseudo, gt, lo_list, hi_list, bs),
        "2m + device statistic, median thr": lambda: pseudo_label_hit_rate(*tr._last_pseudo, gt, thr_mid[0], thr_mid[1], bs, True),
        "3m + host path, median thr": lambda: host_with_gt(*tr._last_pseudo, gt, lo_list, hi_mid, bs),
        "4  + torch-op chain, without gt": lambda: torch_chain_without_gt(*tr._last_pseudo, lo_list, hi_list, bs),
        "5  + device statistic, without gt": lambda: tr.pseudo_label_hit_rate(with_gt=False),
    }
    for fn in stats.values():
        step()
        fn()
    torch.cuda.synchronize()

    # the numbers themselves, on the last step's table, before any time is reported
    t9, valid = tr._last_pseudo
    t9_h, valid_h, gt_h = t9.cpu().numpy(), valid.cpu().numpy(), gt.cpu().numpy()
    want1 = pr.hit_rate(t9_h, valid_h, gt_h, lo_list, hi_list, bs, True)
    want0 = pr.hit_rate(t9_h, valid_h, gt_h, lo_list, hi_list, bs, False)
    got1 = torch.stack(list(tr.pseudo_label_hit_rate(gt, with_gt=True).values())).tolist()
    got0 = torch.stack(list(tr.pseudo_label_hit_rate(with_gt=False).values())).tolist()
    assert got1 == want1.tolist(), (got1, want1.tolist())
    assert got0 == want0.tolist(), (got0, want0.tolist())
    assert host_with_gt(t9, valid, gt, lo_list, hi_list, bs).tolist() == want1.tolist()
    assert torch_chain_without_gt(t9, valid, lo_list, hi_list, bs).tolist() == want0.tolist()
    want_m = pr.hit_rate(t9_h, valid_h, gt_h, lo_list, hi_mid, bs, True)
    got_m = torch.stack(list(pseudo_label_hit_rate(t9, valid, gt, thr_mid[0], thr_mid[1], bs, True).values())).tolist()
    assert got_m == want_m.tolist(), (got_m, want_m.tolist())
    assert host_with_gt(t9, valid, gt, lo_list, hi_mid, bs).tolist() == want_m.tolist()
    rel, unc = pr.split_rows(t9_h, valid_h, lo_list, hi_list)
    unc_m = pr.split_rows(t9_h, valid_h, lo_list, hi_mid)[1]

    per_step = {k: [] for k in stats}
    for _ in range(a.rounds):
        for name, fn in stats.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step()
                fn()
            torch.cuda.synchronize()
            per_step[name].append((time.perf_counter() - t0) / a.steps * 1e3)
    alone = {k: [] for k in stats}
    for name, fn in stats.items():
        for _ in range(20):
            step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            alone[name].append((time.perf_counter() - t0) * 1e3)

    med = {k: statistics.median(v) for k, v in per_step.items()}
    base = "1  step, no statistic"
    spread = max(per_step[base]) - min(per_step[base])
    lines = [
        f"device {torch.cuda.get_device_name(0)}; torch {torch.__version__}",
        f"step: v5l-ssod {B}+{B} images at {S}, bf16, eager; table {t9.shape[0]} rows, {int(valid_h.sum())} valid, {int(rel.sum())} reliable, "
        f"{int(unc.sum())} uncertain; ground truth {gt.shape[0]} labels ({gt.shape[0] / B:.1f} per image)",
        f"numbers (device == host helper, exact): with gt {got1}",
        f"                                        without  {got0}",
        f"                                        with gt, upper threshold {mid:.4f} (median): {int(unc_m.sum())} uncertain rows, {got_m}",
        f"ms per step over {a.steps} steps, {a.rounds} rounds alternated; isolated = the statistic alone between two synchronisations, median of 20",
    ]
    for name in stats:
        lines.append(f"  ({name:<38}) median {med[name]:8.3f} ms   all {[round(v, 3) for v in per_step[name]]}   "
                     f"isolated {statistics.median(alone[name]):8.3f} ms")
    keys = list(stats)
    d2, d3, d2m, d3m, d4, d5 = (med[k] - med[base] for k in keys[1:2] + keys[3:])
    lines += [
        f"run-to-run spread of leg 1 (max - min of its rounds): {spread:.3f} ms",
        f"leg 2 - leg 1 = {d2:+.3f} ms per step: {'within' if abs(d2) <= spread else 'OUTSIDE'} the spread of leg 1",
        f"leg 3 - leg 1 = {d3:+.3f} ms per step: leg 2 is {'below' if d2 < d3 else 'NOT below'} leg 3",
        f"leg 2m - leg 1 = {d2m:+.3f} ms per step ({'within' if abs(d2m) <= spread else 'OUTSIDE'} the spread of leg 1), leg 3m - leg 1 = "
        f"{d3m:+.3f} ms per step: leg 2m is {'below' if d2m < d3m else 'NOT below'} leg 3m",
        f"leg 4 - leg 1 = {d4:+.3f} ms, leg 5 - leg 1 = {d5:+.3f} ms per step (without ground truth: torch-op chain vs kernel)",
        "clocks (read only):", clocks(),
    ]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
