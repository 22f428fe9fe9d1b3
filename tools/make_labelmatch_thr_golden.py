"""Write tests/golden/labelmatch_thresholds.npz: a seeded two-epoch score log and what the LIVE reference computes from it at the end
of each epoch.

The reference is imported through oracle/ref_loader.py (nothing of it is copied): its ``LabelMatch.update_epoch_cls_thr``
(utils/labelmatch.py:191-240) runs on ``score_list_epoch`` filled with the fixture's pairs, as :287 fills it.  The mixture it fits per
class (``gmm_policy`` :138-189) is recorded by wrapping ``sklearn.mixture.GaussianMixture`` while it runs: n_iter_, weights_, means_,
covariances_.  Needs the reference tree and sklearn, so it runs in the build container only (CPU):

    python tools/make_labelmatch_thr_golden.py

The log is tests.labelmatch_thr_ref.synth's (class sizes 0 .. 5000 over ten classes, bimodal / skewed / constant / two-decimal
scores, scores of exactly 1.0 and exactly nms_conf_thres, pairs of class -1 and nc, shuffled); the second epoch permutes the class
sizes so that cls_num_total / (epoch + 1) is the binding rank in some classes.  The generator ASSERTS, and moves on to the next
seed until all hold:
  (a) no class reaches 100 EM iterations;
  (b) at least one fitted class ends with nothing assigned to the upper component;
  (c) at least one class has thr_high > 0 and at least one thr_high == 0;
  (d) the numpy helper reproduces the reference: thresholds and n_iter exactly; and still does so, on every class, with every exp
      moved by up to 4 units in the last place and every class's scores in a permuted order (so that a last-bit difference of a
      device's exp, or another reduction tree, moves no result).  The worst relative change of the six mixture parameters under
      that perturbation is stored as ``self_dev``: the tests' tolerance on the parameters is 100 x self_dev."""
import io
import logging
import os
import sys
from contextlib import redirect_stdout

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_loader  # noqa: E402
from oracle.make_golden import SSOD_YAML, TINY  # noqa: E402
from tests import labelmatch_thr_ref as lr  # noqa: E402

SEED0 = 20261019
TRIALS = 3           # perturbed / permuted repetitions per epoch


class Unfit(Exception):
    pass


def need(ok, why):
    if not ok:
        raise Unfit(why)


def reference_epochs(cfg, logs):
    """[(thr_high, thr_low, n_iter, gmm)] per epoch from the live reference"""
    import sklearn.mixture as skm
    from utils.labelmatch import LabelMatch
    fitted = []

    class Recording(skm.GaussianMixture):
        def fit(self, X, y=None):
            r = super().fit(X, y)
            fitted.append(self)
            return r

    nc = lr.NC
    lm = LabelMatch(cfg, 100, 5, cls_ratio_gt=np.full(nc, 1.0 / nc))
    logging.getLogger().setLevel(logging.WARNING)
    real, out = skm.GaussianMixture, []
    skm.GaussianMixture = Recording
    try:
        for epoch, (conf, cls) in enumerate(logs):
            for s, c in zip(conf, cls):
                if 0 <= c < nc:                                    # a class outside the range never reaches :287
                    lm.score_list_epoch[int(c)].append(float(s))
            sizes = [len(v) for v in lm.score_list_epoch]
            del fitted[:]
            with redirect_stdout(io.StringIO()):
                lm.update_epoch_cls_thr(epoch)
            n_iter, gmm = np.zeros(nc, np.int32), np.zeros((nc, 6))
            it = iter(fitted)
            for c in range(nc):
                if sizes[c] >= lr.MIN_FIT:
                    g = next(it)
                    n_iter[c] = g.n_iter_
                    gmm[c] = np.concatenate((g.weights_, g.means_.reshape(-1), g.covariances_.reshape(-1)))
            assert next(it, None) is None
            out.append((np.array(lm.cls_thr_high, np.float64), np.array(lm.cls_thr_low, np.float64), n_iter, gmm))
    finally:
        skm.GaussianMixture = real
    return out


def main():
    nc = lr.NC
    cfg = ref_loader.get_cfg(SSOD_YAML, TINY + ["Dataset.nc", nc, "SSOD.pseudo_label_type", "LabelMatch", "SSOD.resample_low_percent",
                                                lr.RESAMPLE_LOW_PERCENT, "Dataset.names", [str(i) for i in range(nc)]])
    cfg.freeze()
    lo, hi, pct = cfg.SSOD.ignore_thres_low, cfg.SSOD.ignore_thres_high, cfg.SSOD.resample_low_percent
    for seed in range(SEED0, SEED0 + 50):
        logs = [lr.synth(seed, e, cfg.SSOD.nms_conf_thres) for e in (0, 1)]
        try:
            ref = reference_epochs(cfg, logs)
            total, mine, self_dev = np.zeros(nc, np.int64), [], 0.0
            for epoch, (conf, cls) in enumerate(logs):
                high, low, n_iter, gmm = ref[epoch]
                m = lr.thresholds(conf, cls, nc, epoch, lo, hi, pct, total)
                need(int(n_iter.max()) < lr.MAX_ITER, "(a) a class ran 100 iterations")
                need(np.array_equal(m["thr_high"], high) and np.array_equal(m["thr_low"], low) and np.array_equal(m["n_iter"], n_iter),
                     f"(d) helper != reference: {m['thr_high']} {high} {m['n_iter']} {n_iter}")
                need(not m["status"].any(), "a rank outside its segment")
                fit = n_iter > 0
                dev0 = float(np.abs(m["gmm"][fit] / gmm[fit] - 1).max())
                for t in range(TRIALS):
                    rng = np.random.default_rng([seed, epoch, t, 7])
                    p = lr.thresholds(conf, cls, nc, epoch, lo, hi, pct, total, exp=lr.ulp_noise_exp(rng), rng=rng)
                    need(np.array_equal(p["thr_high"], high) and np.array_equal(p["thr_low"], low) and np.array_equal(p["n_iter"], n_iter),
                         "(d) a 4-ulp perturbation of exp moves a result")
                    self_dev = max(self_dev, float(np.abs(p["gmm"][fit] / gmm[fit] - 1).max()))
                print(f"seed {seed} epoch {epoch}: helper vs sklearn parameters {dev0:.2e}; n_iter {n_iter.tolist()}\n"
                      f"   high {high.tolist()}\n   low  {low.tolist()}\n   assigned to the upper component {m['assigned1'].tolist()}")
                need(dev0 <= 100 * self_dev, f"helper's parameters {dev0:.2e} off sklearn's, self_dev {self_dev:.2e}")
                total = m["cls_num_total"]
                mine.append(m)
            highs = np.concatenate([r[0] for r in ref])
            fitted = np.concatenate([r[2] for r in ref]) > 0
            need((highs > 0).any() and (highs == 0).any(), "(c) thr_high")
            need((fitted & (np.concatenate([m["assigned1"] for m in mine]) == 0)).any(), "(b) every fitted class uses the upper component")
        except Unfit as e:
            print(f"seed {seed}: {e}")
            continue
        break
    else:
        raise SystemExit("no seed fits")
    out = dict(nc=np.int64(nc), seed=np.int64(seed), self_dev=np.float64(self_dev),
               cfg=np.array([cfg.SSOD.nms_conf_thres, lo, hi, pct], np.float64))
    for epoch, ((conf, cls), (high, low, n_iter, gmm)) in enumerate(zip(logs, ref)):
        out.update({f"conf{epoch}": conf, f"cls{epoch}": cls, f"thr_high{epoch}": high, f"thr_low{epoch}": low,
                    f"n_iter{epoch}": n_iter, f"gmm{epoch}": gmm})
    path = os.path.join(ROOT, "tests", "golden", "labelmatch_thresholds.npz")
    np.savez_compressed(path, **out)
    print(f"self_dev {self_dev:.3e}\n{path} {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
