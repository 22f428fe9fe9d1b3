"""TEST INFRASTRUCTURE -- numpy restatement of LabelMatch's end-of-epoch thresholds (reference utils/labelmatch.py:188-240 with
gmm_policy :138-189 and the sklearn.mixture.GaussianMixture fit it runs), the yardstick of csrc/labelmatch.hip.

  segments    the logged (class, confidence) pairs -> per-class scores sorted descending, one after the other, and the offsets;
  fit         the two-component EM, fp64: w = (1/2, 1/2), mu = (min, max), var = (1, 1);
              E: lp_k = -(log 2pi + (x - mu_k)^2 / var_k) / 2 - log(var_k) / 2 + log w_k, norm = logsumexp_k lp_k, log_resp = lp - norm;
              M, r = exp(log_resp): nk = sum r + 10 eps, mu = sum r x / nk, var = sum r (x - mu_new)^2 / nk + 1e-6, w = nk / n
              renormalised; lower bound = mean norm of the E-step BEFORE the M-step; stop at |change| < 1e-3 or after 100 iterations;
              then one more E-step;
  policy      'high' with given_gt_thr 0.0;
  thresholds  one epoch's end over every class.

tests/golden/labelmatch_thresholds.npz (tools/make_labelmatch_thr_golden.py) pins this file on the LIVE reference and sklearn:
thresholds and n_iter_ exactly, the fitted parameters within 100 x the fixture's self_dev.  ``synth`` is the fixture's generator."""
import numpy as np

LOG_2PI = float(np.log(2.0 * np.pi))
MAX_ITER, TOL, REG_COVAR, MIN_FIT = 100, 1e-3, 1e-6, 4
OK, RANK_OUT_OF_SEGMENT = 0, 1

NC = 10
# class sizes of the two epochs: every segment boundary of the sorted log falls inside a wave (no multiple of 64) and inside a
# sort tile; the second epoch permutes them so that int(cls_num_total / (epoch + 1)) is the smaller rank in some classes
SIZES = ((65, 0, 1, 3, 4, 63, 257, 64, 1000, 5000), (5000, 3, 1000, 0, 257, 4, 64, 65, 63, 1))
SHAPES = ("bimodal", "skewed", "rounded", "bimodal", "skewed", "edges", "constant", "rounded", "skewed", "bimodal")
RESAMPLE_LOW_PERCENT = 0.9


def _scores(rng, shape, n, conf_thres):
    lo = float(np.float32(conf_thres))
    if shape == "constant":
        return np.full(n, 0.4375, np.float32)
    if shape == "skewed":
        return (0.1 + 0.9 * rng.beta(1.2, 4.0, n)).astype(np.float32)
    top = rng.random(n) < 0.4
    s = np.where(top, rng.normal(0.8, 0.07, n), rng.normal(0.25, 0.08, n))
    s = np.clip(s, lo + 1e-3, 0.999).astype(np.float32)
    if shape == "rounded":
        s = np.round(s.astype(np.float64), 2).astype(np.float32)
    if shape == "edges" and n >= 3:
        s[0] = s[1] = 1.0
        s[2] = np.float32(conf_thres)
    return s


def synth(seed, epoch, conf_thres):
    """one epoch's log: (conf fp32, cls int32), shuffled, with a few pairs of class -1 and NC that every consumer drops"""
    rng = np.random.default_rng([seed, epoch])
    conf, cls = [], []
    for c, n in enumerate(SIZES[epoch]):
        conf.append(_scores(rng, SHAPES[c], n, conf_thres))
        cls.append(np.full(n, c, np.int32))
    conf.append(rng.uniform(0.2, 0.9, 10).astype(np.float32))
    cls.append(np.array([-1] * 5 + [NC] * 5, np.int32))
    conf, cls = np.concatenate(conf), np.concatenate(cls)
    p = rng.permutation(conf.shape[0])
    return conf[p], cls[p]


def segments(conf, cls, nc):
    conf, cls = np.asarray(conf, np.float32), np.asarray(cls)
    parts = [np.sort(conf[cls == c])[::-1] for c in range(nc)]
    seg = np.concatenate(([0], np.cumsum([p.shape[0] for p in parts]))).astype(np.int64)
    return np.concatenate(parts).astype(np.float32), seg


def ulp_noise_exp(rng, k=4):
    """np.exp with every result moved by up to k units in the last place"""
    def f(a):
        v = np.exp(a)
        step = rng.integers(-k, k + 1, v.shape)
        return np.where(v > 1e-300, (v.view(np.int64) + step).view(np.float64), v)
    return f


def _e_step(x, w, mu, var, exp):
    lp = np.stack([-0.5 * (LOG_2PI + (x - mu[k]) * (x - mu[k]) / var[k]) - 0.5 * np.log(var[k]) + np.log(w[k]) for k in (0, 1)], 1)
    m = lp.max(1)
    norm = m + np.log(exp(lp[:, 0] - m) + exp(lp[:, 1] - m))
    return norm, lp - norm[:, None]


def fit(x, exp=np.exp):
    """x (n >= 4) fp64 in any order -> dict(w, mu, var, n_iter, norm, log_resp); norm / log_resp of the final E-step, in x's order"""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    w, mu, var = np.array([0.5, 0.5]), np.array([x.min(), x.max()]), np.array([1.0, 1.0])
    prev, n_iter = -np.inf, MAX_ITER
    for it in range(1, MAX_ITER + 1):
        norm, log_resp = _e_step(x, w, mu, var, exp)
        bound = norm.sum() / n
        r = exp(log_resp)
        nk = r.sum(0) + 10.0 * np.finfo(np.float64).eps
        mu = (r * x[:, None]).sum(0) / nk
        d = x[:, None] - mu
        var = (r * (d * d)).sum(0) / nk + REG_COVAR
        w = nk / n
        w = w / (w[0] + w[1])
        change, prev = bound - prev, bound
        if abs(change) < TOL:
            n_iter = it
            break
    norm, log_resp = _e_step(x, w, mu, var, exp)
    return dict(w=w, mu=mu, var=var, n_iter=n_iter, norm=norm, log_resp=log_resp)


def policy_high(x, f, given=0.0):
    assign = f["log_resp"][:, 1] > f["log_resp"][:, 0]                 # argmax, a tie goes to component 0
    if not assign.any():
        return given, 0
    top = f["norm"][assign].max()
    x_top = x[assign & (f["norm"] == top)].max()
    return max(given, float(x[assign & (x >= x_top)].min())), int(assign.sum())


def class_thresholds(s, exp=np.exp, order=None):
    """s: one class's scores -> (thr_high for a non-empty class, n_iter, gmm (6,), samples assigned to component 1)"""
    x = np.asarray(s, np.float64)
    if order is not None:
        x = x[order]
    if x.shape[0] < MIN_FIT:
        return 0.0, 0, np.zeros(6), 0
    f = fit(x, exp)
    thr, n1 = policy_high(x, f)
    return thr, f["n_iter"], np.concatenate((f["w"], f["mu"], f["var"])), n1


def thresholds(conf, cls, nc, epoch, ignore_low, ignore_high, low_percent, cls_num_total, exp=np.exp, rng=None):
    """one end of an epoch.  cls_num_total (nc) is NOT modified; rng: fit every class on a permutation of its scores"""
    sorted_conf, seg = segments(conf, cls, nc)
    out = dict(thr_high=np.zeros(nc), thr_low=np.zeros(nc), n_per_class=np.diff(seg), n_iter=np.zeros(nc, np.int32),
               status=np.zeros(nc, np.int32), gmm=np.zeros((nc, 6)), assigned1=np.zeros(nc, np.int64),
               cls_num_total=np.asarray(cls_num_total, np.int64) + np.diff(seg), sorted_conf=sorted_conf, seg_offset=seg)
    for c in range(nc):
        s = sorted_conf[seg[c]:seg[c + 1]]
        n = s.shape[0]
        if n == 0:
            out["thr_high"][c], out["thr_low"][c] = ignore_high, ignore_low
            continue
        pos = min(int(float(out["cls_num_total"][c]) / (epoch + 1)), int(n * low_percent))
        if pos < 0 or pos >= n:
            out["status"][c], out["thr_low"][c] = RANK_OUT_OF_SEGMENT, ignore_low
        else:
            out["thr_low"][c] = max(ignore_low, float(s[pos]))
        order = rng.permutation(n) if rng is not None else None
        out["thr_high"][c], out["n_iter"][c], out["gmm"][c], out["assigned1"][c] = class_thresholds(s, exp, order)
    return out
