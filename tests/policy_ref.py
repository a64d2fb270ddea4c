"""Host reference for log_prob_items and the off-policy estimators, shared by
tests/test_policy_host.py and tests/test_hip_policy.py.  Nothing here touches a GPU; everything is numpy float64 over the
float64 oracle logits of tests/sampling_ref.py."""
import numpy as np

from tests import sampling_ref as R

NEG_INF = float("-inf")
ROWS = R.DIST["rows"]   # logged rows of the end-to-end test
SIGMAS = 4.9            # the two-sided 1e-6 level of a normal deviate: the significance the chi-square tests here use
FP32_SLACK = 1e-3       # what the fp32 logits move the weights' mean by, at most (the issue's figure)


def policy_stats(z):
    """z [I] float64, logit / tau of the eligible items -> (log-softmax [I], logsumexp, entropy in nats, E_p|log p + H|:
    the 1-norm of the entropy's gradient in z, dH/dz_i = -p_i (log p_i + H))."""
    z = np.asarray(z, dtype=np.float64)
    if z.size == 0:
        return z, NEG_INF, 0.0, 0.0
    lp = R.log_softmax(z)
    p = np.exp(lp)
    lse = float(z.max() + np.log(np.exp(z - z.max()).sum()))
    H = float(-(p * lp).sum())
    return lp, lse, H, float((p * np.abs(lp + H)).sum())


def entropy_of_log_probs(lp):
    """-sum exp(lp) lp in float64 over a row of log-probabilities."""
    lp = np.asarray(lp, dtype=np.float64)
    return float(-(np.exp(lp) * lp).sum())


def entropy_format_tol(n_eligible: int) -> float:
    """What the reduction's fp32 arithmetic may move the entropy by, from the formats: a few ulps (2^-24) each for exp2f,
    the merges' expf, logf and the division, against values of size at most 1 + log n."""
    return 64 * 2.0 ** -24 * (1.0 + np.log(max(n_eligible, 1)))


def estimates(log_ratio, rewards, clip=None):
    """off_policy_estimate's closed forms in numpy float64."""
    w = np.exp(np.asarray(log_ratio, dtype=np.float64))
    if clip is not None:
        w = np.minimum(w, clip)
    r = np.asarray(rewards, dtype=np.float64)
    return dict(ips=(w * r).mean(), snips=(w * r).sum() / w.sum(), ess=w.sum() ** 2 / (w * w).sum(), max_weight=w.max(),
                n=len(w))


def e2e_inputs():
    """The end-to-end test's figures from the oracle alone: sampling_ref.dist_inputs()'s user, logging temperature tau_A =
    its tau, target temperature tau_A / 2, reward 1 where the item's oracle logit is above the eligible median.  ->
    dict(geo, cfg, P, attrs, batch, ids, tau_a, tau_b, reward [I], p_a, p_b, v_a, v_b, w [I], sd, band): V = sum p r, w
    = p_b / p_a, sd the standard deviation of the IPS mean over ROWS rows, band = SIGMAS sd + FP32_SLACK."""
    geo, cfg, P, attrs, batch, ids, lg, tau, p_a = R.dist_inputs()
    tau_a = tau
    tau_b = float(np.float32(tau_a / 2.0))
    p_b = np.exp(R.log_softmax(lg / tau_b))
    reward = (lg > np.median(lg)).astype(np.float64)
    w = p_b / p_a
    v_a, v_b = float((p_a * reward).sum()), float((p_b * reward).sum())
    sd = float(np.sqrt(((p_a * (w * reward) ** 2).sum() - v_b ** 2) / ROWS))
    return dict(geo=geo, cfg=cfg, P=P, attrs=attrs, batch=batch, ids=ids, logits=lg, tau_a=tau_a, tau_b=tau_b,
                reward=reward, p_a=p_a, p_b=p_b, v_a=v_a, v_b=v_b, w=w, sd=sd, band=SIGMAS * sd + FP32_SLACK)
