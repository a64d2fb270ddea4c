"""Host reference for recommend_sampled (the noise contract of include/carca_hip.h restated in numpy),
shared by tests/test_sampled_host.py and tests/test_hip_sampled.py.  Nothing here touches a GPU.

The hash, every variable a numpy uint32 (arithmetic mod 2^32), seed and key 64 bits (the key an int64 reinterpreted):
    mix32(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16
    hu = mix32(seed_lo ^ (key_lo * 0x9E3779B1));   hu = mix32(hu ^ seed_hi ^ (key_hi * 0x85EBCA77))
    h  = mix32(hu ^ (item * 0xC2B2AE3D))
    U  = ((h >> 9) + 0.5) * 2^-23   -- 23 hash bits, U in [2^-24, 1 - 2^-24];   g = -log(-log(U)) in float64
The noise belongs to (seed, user key, item id): never to a column or a batch row."""
import math

import numpy as np
import torch

from oracle import carca_oracle as O

G, N_ATTRS = 24, 12
G_MIN = -math.log(24 * math.log(2.0))               # U = 2^-24
G_MAX = -math.log(-math.log1p(-2.0 ** -24))         # U = 1 - 2^-24
MARGIN_FLOOR = 1e-4   # fp32 rounding of z, g and z + g on the device, for |z| up to a few hundred
E_KERNEL_ULPS = 16    # fp32 arithmetic in front of the link, in ulps (2^-24) of the largest logit magnitude (e_bound)
AMBIGUOUS_CAP = 0.02

# name -> (d, H, embedding, decoder, encoding, residual_ca, n_ctx, n_blocks, l2): tests/test_hip_retrieve.py's
GEOS = {
    "ca64x4-all": (64, 4, "all", "ca", "identity", True, 6, 1, False),
    "dot64x2": (64, 2, "all", "dot", "identity", True, 6, 1, False),
    "wdot96x2-l2": (96, 2, "all", "wdot", "positional", True, 6, 1, True),
}
SIZES = (33, 257, 1000)       # the issue's sizes: one chunk of the perturb pass each (csrc/sampled_select.h: SP_CHUNK = 1024)
# Sizes that give the perturb pass 5 and 9 chunks -- more chunks than a workgroup has waves, parts of unequal length, a last
# chunk of 3 and of 809 columns -- and, being 3 and 1 mod 4, rows and chunk starts off the 16-byte boundary.
BIG_SIZES = (4099, 9001)
B, L = 5, 9
# The order test's temperatures: (largest - smallest oracle logit of the inputs) / R, so z spans R whatever the decoder's
# scale (the dot decoder's logits span 60, the l2 decoder's 0.8).  A catalogue of 1000 items under noise alone packs its
# keys densely enough that the margin's floor leaves 2 % of adjacent pairs out by itself; a z spread well past the
# noise's (g_max - g_min = 19.4) thins them (test_sampled_host shows the share under the cap for these R).
ORDER_SPANS = (64.0, 256.0)
DIST = dict(geo="ca64x4-all", n=33, L=5, rows=4096, k=2, seed=20261020)


# ---- the noise -------------------------------------------------------------------------------------------------------
def mix32(x):
    x = np.asarray(x, dtype=np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def user_hash(seed: int, keys):
    """hu [U] (uint32) of the int64 keys under `seed` (any int: taken mod 2^64)."""
    seed = int(seed) % (1 << 64)
    k = np.asarray(keys, dtype=np.int64).astype(np.uint64)
    lo, hi = (k & np.uint64(0xFFFFFFFF)).astype(np.uint32), (k >> np.uint64(32)).astype(np.uint32)
    with np.errstate(over="ignore"):
        h = mix32(np.uint32(seed & 0xFFFFFFFF) ^ (lo * np.uint32(0x9E3779B1)))
        return mix32(h ^ np.uint32(seed >> 32) ^ (hi * np.uint32(0x85EBCA77)))


def item_hash(hu, items):
    """h [U, I] (uint32): every 32-bit hash value of the contract."""
    with np.errstate(over="ignore"):
        it = np.asarray(items, dtype=np.int64).astype(np.uint32) * np.uint32(0xC2B2AE3D)
        return mix32(np.asarray(hu, dtype=np.uint32)[:, None] ^ it[None, :])


def uniform(h):
    return ((np.asarray(h, dtype=np.uint32) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def gumbel(seed: int, keys, items):
    """g [U, I] float64."""
    return -np.log(-np.log(uniform(item_hash(user_hash(seed, keys), items))))


# ---- the draw ----------------------------------------------------------------------------------------------------------
def perturbed_order(z, ids, seed: int, key: int):
    """z [I] float64 (logit / tau of the ELIGIBLE items), ids [I] their item ids -> (ids in perturbed order: key z + g
    descending, ties to the smaller id; the sorted keys)."""
    ids = np.asarray(ids, dtype=np.int64)
    keys = np.asarray(z, dtype=np.float64) + gumbel(seed, [key], ids)[0]
    order = np.lexsort((ids, -keys))
    return ids[order], keys[order]


def log_softmax(z):
    z = np.asarray(z, dtype=np.float64)
    m = z.max()
    return z - (m + np.log(np.exp(z - m).sum()))


def pl_marginals(p):
    """p [I] float64, sum 1 -> (first-pick, second-pick) exact Plackett-Luce marginals: P(second = j) = sum_{i != j}
    p_i p_j / (1 - p_i)."""
    p = np.asarray(p, dtype=np.float64)
    w = p / (1.0 - p)
    return p, p * (w.sum() - w)


def chi2_critical(dof: int, alpha: float) -> float:
    """The chi-square value whose upper tail is alpha at `dof` degrees of freedom, from the regularised upper incomplete
    gamma function (sf(x) = Q(dof / 2, x / 2)) by bisection: computed, never a table value."""
    a = torch.tensor(dof / 2.0, dtype=torch.float64)
    lo, hi = 0.0, 10.0 * dof + 200.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if float(torch.special.gammaincc(a, torch.tensor(mid / 2.0, dtype=torch.float64))) > alpha:
            lo = mid
        else:
            hi = mid
    return hi


def chi2_stat(counts, probs, total: int):
    """Pearson's statistic of observed counts against expected total * probs, bins with expected < 5 merged into one
    (and that one into the smallest other bin while it is still short) -> (statistic, degrees of freedom)."""
    exp = np.asarray(probs, dtype=np.float64) * total
    obs = np.asarray(counts, dtype=np.float64)
    small = exp < 5
    e, o = list(exp[~small]), list(obs[~small])
    if small.any():
        es, os_ = exp[small].sum(), obs[small].sum()
        if es < 5 and e:
            j = int(np.argmin(e))
            e[j] += es
            o[j] += os_
        else:
            e.append(es)
            o.append(os_)
    e, o = np.array(e), np.array(o)
    return float(((o - e) ** 2 / e).sum()), len(e) - 1


# ---- inputs: tests/test_hip_retrieve.py's _setup, the oracle half and the device half apart ---------------------------
def oracle_setup(geo, L, B, n_items, seed=0):
    """-> (cfg, P, attrs, (p_x, p_c, ctx)): float64 parameters and a batch drawn as test_hip_retrieve._setup draws them
    (B > 2 holds an empty and a one-slot profile)."""
    d, H, emb, dec, enc, res_ca, n_ctx, nb, l2 = GEOS[geo]
    cfg = O.CarcaConfig(d=d, H=H, n_blocks=nb, residual_ca=res_ca, encoding=enc, embedding=emb, decoder=dec, l2_norm=l2)
    P = O.perturb_params(O.init_params(cfg, n_items, G, n_ctx, N_ATTRS, L, seed=seed, dtype=torch.float64), seed=seed + 1)
    rng = np.random.default_rng(seed + 7)
    attrs = torch.from_numpy(rng.random((n_items, N_ATTRS))).double()
    attrs[0] = 0
    p_x = torch.zeros(B, L, dtype=torch.int64)
    for b in range(B):
        ell = 0 if (b == 1 and B > 2) else 1 if (b == 2 and B > 2) else int(rng.integers(1, L + 1))
        if ell:
            p_x[b, L - ell:] = torch.from_numpy(rng.integers(1, n_items, size=ell))
    p_c = torch.from_numpy(rng.random((B, L, n_ctx))).double() * (p_x != 0).unsqueeze(-1)
    ctx = torch.from_numpy(rng.random((B, n_ctx))).double()
    return cfg, P, attrs, (p_x, p_c, ctx)


def device_model(geo, P, attrs, n_items, L):
    from tests.model_util import build_model

    d, H, emb, dec, enc, res_ca, n_ctx, nb, l2 = GEOS[geo]
    model = build_model(dict(d=d, H=H, n_blocks=nb, encoding=enc, residual_ca=res_ca, embedding=emb, decoder=dec,
                             l2_norm=l2), n_items, G, n_ctx, N_ATTRS, L)
    model.load_state_dict({k: v.float() for k, v in P.items()}, strict=True)
    model = model.cuda().eval()
    if hasattr(model.embeds, "register_attr_table"):
        model.embeds.register_attr_table(attrs.float().cuda())
    return model


def unlink(y, geo, y_neg=None):
    """The raw logit behind a score, in float64: 2 y - 1 for the l2 decoder, else log(y / (1 - y)) -- with 1 - y taken as
    y_neg = sigmoid(-logit) where the caller has it: near y = 1 the subtraction 1 - y keeps few digits of the logit
    (none past logit 37, where y rounds to 1), while sigmoid(-logit) keeps them all."""
    y = y.double()
    if GEOS[geo][8]:
        return 2.0 * y - 1.0
    return torch.log(y) - torch.log(y_neg.double() if y_neg is not None else 1.0 - y)


def e_bound(geo, logits) -> float:
    """What |logit64(score_items) - oracle logit| can reach over the pairs with |logit| < 8 of these oracle logits, from
    the number formats.  The sigmoid link is 1 / (1 + exp(-logit)) in fp32: the sum lies in [1, 2) and rounds by up to
    2^-24, the quotient lies below 1 and rounds by up to 2^-25, so the score is off by up to 1.5 * 2^-24 and the logit read
    back from it by that over y (1 - y) -- 2.7e-4 at |logit| = 8.  The l2 link (y + 1) / 2 rounds by 2^-25, twice that in
    the logit.  To this come E_KERNEL_ULPS ulps of the largest logit magnitude of the inputs for the fp32 arithmetic in
    front of the link (a small logit of the dot decoder is the sum of terms as large as its large ones)."""
    a = np.abs(np.asarray(logits, dtype=np.float64))
    top = float(a[a < 8].max()) if (a < 8).any() else 0.0
    y = 1.0 / (1.0 + math.exp(-top))
    return E_KERNEL_ULPS * 2.0 ** -24 * max(1.0, float(a.max())) + (2.0 ** -24 if GEOS[geo][8] else 1.5 * 2.0 ** -24 / (y * (1.0 - y)))


def order_taus(logits):
    """The order test's temperatures for these oracle logits [B, n_items] (column 0 left out), as fp32 values."""
    y = np.asarray(logits, dtype=np.float64)[:, 1:]
    return [float(np.float32((y.max() - y.min()) / r)) for r in ORDER_SPANS]


def oracle_logits(geo, cfg, P, attrs, batch, n_items):
    """[B, n_items] float64 raw logits of the float64 oracle (column 0, the padding item, is 0 and never eligible): the
    scores as tests/test_hip_retrieve.py::_oracle_scores gets them, the link inverted in float64 (unlink).  The dot
    decoder's logits reach 30 and more, so its sigmoid(-logit) comes from the oracle too: its own dot_decoder over the
    traced encoder output and the NEGATED traced item embeddings."""
    p_x, p_c, ctx = batch
    nb = p_x.shape[0]
    ids = torch.cat([torch.arange(1, n_items), torch.zeros(1, dtype=torch.int64)]).expand(nb, -1)
    o_c = ctx.unsqueeze(1).expand(nb, n_items, ctx.shape[1])
    trace = {}
    y = O.carca_forward(P, cfg, (p_x, attrs[p_x], p_c), [(ids, attrs[ids], o_c)], training=False, trace=trace)
    y_neg = None
    if cfg.decoder != "ca" and not GEOS[geo][8]:
        y_neg = O.dot_decoder(cfg, -trace["o_embed0"], trace["p_final"], False).reshape(nb, n_items)[:, :-1]
    z = unlink(y.reshape(nb, n_items)[:, :-1], geo, y_neg)
    return torch.cat([torch.zeros(nb, 1, dtype=torch.float64), z], 1)


def eligible_ids(p_x_row, n_items, extra=()):
    """Ascending eligible ids of a user under exclude="profile" plus `extra`."""
    out = set(range(1, n_items)) - set(int(v) for v in p_x_row.tolist()) - set(int(v) for v in extra)
    return np.array(sorted(out), dtype=np.int64)


def order_margin(e: float, tau: float) -> float:
    return 2.0 * e / tau + MARGIN_FLOOR


def dist_inputs():
    """The distribution test's user: -> (geo, cfg, P, attrs, batch of ONE user, eligible ids, logits of them, tau, p).
    tau = (largest - smallest eligible oracle logit) / 3: z spans 3, so with 28 or more eligible items the largest
    probability is far below 0.5 (asserted by both tests)."""
    geo, n = DIST["geo"], DIST["n"]
    cfg, P, attrs, batch = oracle_setup(geo, DIST["L"], 1, n, seed=3)
    y = oracle_logits(geo, cfg, P, attrs, batch, n)[0].numpy()
    ids = eligible_ids(batch[0][0], n)
    lg = y[ids]
    tau = float(np.float32((lg.max() - lg.min()) / 3.0))
    p = np.exp(log_softmax(lg / tau))
    return geo, cfg, P, attrs, batch, ids, lg, tau, p


def dist_check(first, second, ids, p, rows):
    """first / second [rows]: the drawn ids.  Both chi-square tests at significance 1e-6 -> the figures, for printing."""
    p1, p2 = pl_marginals(p)
    out = []
    for name, drawn, q in (("first", first, p1), ("second", second, p2)):
        counts = np.array([(np.asarray(drawn) == i).sum() for i in ids])
        assert counts.sum() == rows, name  # every draw is an eligible id
        stat, dof = chi2_stat(counts, q, rows)
        crit = chi2_critical(dof, 1e-6)
        out.append((name, stat, dof, crit))
    return out
