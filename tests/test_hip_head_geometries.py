"""Every head geometry of the fused attention kernels, and every (d, H) they are not built for, in training and evaluation
against torch.autograd over the CPU oracle in fp64.

The fused per-user kernels (sa_block / sa_eval / cross_score / cross_stream and the backward kernels sa_attn_bwd /
cross_attn_bwd) are template instances per (DPI, DHP, H) -- CARCA_ATT_GEOMETRIES in csrc/attn_common.h -- each with its own
compile-time branches (V in LDS or not, one or two head slots in the cross backward, how heads split between two
workgroups, padding inside a head).  Here each of the nine is trained (one step, p = 0, two target groups built as train.py
builds them) and evaluated (N = 1 and N = 101 candidates) at least twice, across profile lengths L = 1, 16, 17, 33, 48, 64,
with users of lengths L, 1, 0, 15, 16, 17 and one with a pad slot inside, under the three attention work splits
(carca_set_tuning key 1: 0 = two workgroups per user at these batch sizes, 1 = one, 3 = the 8-wave scoring workgroup), and
one case at B = 160 (one workgroup per user by default).  (d, H) pairs without a fused kernel run the composed path
(long_profile.py), checked the same way.

Tolerances are the suite's: scores 2e-5, loss 2e-6 relative, every parameter gradient 1e-4 of the tensor's largest entry
(+ a floor of 1e-5 of the module's largest gradient, for the attention key biases whose true gradient is 0)."""
import functools

import pytest
import torch

from oracle import carca_oracle as O
from tests.model_util import assert_all_users_match_oracle, dev, model_from_params
from tests.test_hip_standalone_grad import _P64, _check_params

pytestmark = pytest.mark.gpu

N_ITEMS, N_CTX = 300, 3


def _lengths(B, L):
    """Profile lengths of a batch: L, 1, 0 (empty), 15, 16, 17 where they fit, then L again."""
    want = [L, 1, 0, 15, 16, 17]
    out = [x for x in want if x <= L]
    while len(out) < B:
        out.append(L)
    return out[:B]


def _batch(B, L, N, n_attrs, seed):
    """A batch with controlled profile lengths (left-padded, data.py:113) and, where L >= 3, one pad slot inside the last
    user's profile.  Returns (profile, target): target = N candidates per user (positive first, negatives outside the
    profile, synth_eval_batch)."""
    (p_x, p_a, p_c), target, table = O.synth_eval_batch(B, L, N, N_ITEMS, n_attrs, N_CTX, seed=seed, min_len=L)
    lens = _lengths(B, L)
    for u, ell in enumerate(lens):
        p_x[u, : L - ell] = 0
    if L >= 3 and B >= 7:
        p_x[B - 1, L // 2] = 0
    keep = (p_x != 0)
    return (p_x, table[p_x.long()], p_c * keep[..., None]), target


def _train_targets(profile, seed, n_attrs, n_groups=2):
    """train.py:86-88: groups of N = L targets (a positive and negatives), zeroed where the profile is padding."""
    p_x = profile[0]
    B, L = p_x.shape
    groups = []
    for gi in range(n_groups):
        _, (o_x, o_a, o_c), _ = O.synth_eval_batch(B, L, L, N_ITEMS, n_attrs, N_CTX, seed=seed + 17 * gi, min_len=L)
        groups.append((o_x * (p_x != 0), o_a, o_c))
    y_true = torch.cat([(p_x != 0).int()] + [torch.zeros_like(p_x)] * (n_groups - 1), dim=1)
    o_x = torch.cat([g[0] for g in groups], dim=1)
    return groups, y_true, o_x


def _f64(seg):
    return (seg[0], seg[1].double(), seg[2].double())


def _per_user(y, B, n_groups):
    """[B, sum N] scores; at N = 1 the bare squeeze (carca.py:346) leaves each group [B] and the join [n_groups * B]."""
    return y if y.dim() == 2 else y.view(n_groups, B).t()


@functools.lru_cache(maxsize=None)
def _case(d, H, L, B, nb=1, res_sa=True, res_ca=True, n_attrs=12, g=24, n_groups=2, seed=0):
    """Parameters, batches and the fp64 oracle's answers of one case (computed once, shared by the variants)."""
    cfg = O.CarcaConfig(d=d, H=H, n_blocks=nb, residual_sa=res_sa, residual_ca=res_ca)
    P = O.perturb_params(O.init_params(cfg, N_ITEMS, g, N_CTX, n_attrs, L, seed=seed), seed=seed + 1, scale=0.2)
    profile, _ = _batch(B, L, 1, n_attrs, seed + 2)
    groups, y_true, o_x = _train_targets(profile, seed + 3, n_attrs, n_groups)
    P64 = _P64(P)
    y64 = _per_user(O.carca_forward(P64, cfg, _f64(profile), [_f64(t) for t in groups], training=True), B, n_groups)
    loss64 = O.bce_loss(y64, y_true.double(), O.get_mask(o_x, torch.float64))
    loss64.backward()
    evals = []
    with torch.no_grad():
        for N in (1, 101):
            prof_e, tgt_e = _batch(B, L, N, n_attrs, seed + 5 + N)
            evals.append((prof_e, tgt_e, O.carca_forward(P64, cfg, _f64(prof_e), [_f64(tgt_e)], training=False)))
    return cfg, P, P64, profile, groups, y_true, o_x, y64.detach(), float(loss64.detach()), evals


@pytest.fixture
def composed_calls(monkeypatch):
    """Counts calls of the composed path (long_profile.forward)."""
    from carca_replication_amd import long_profile

    calls = []
    real = long_profile.forward

    def spy(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(long_profile, "forward", spy)
    return calls


@pytest.fixture
def set_variant():
    from carca_replication_amd import _lib

    lib = _lib.load()
    yield lambda v: lib.carca_set_tuning(1, v)
    lib.carca_set_tuning(1, 0)


def _run_case(key, composed_calls, expect_composed):
    from carca_replication_amd import modules as M

    cfg, P, P64, profile, groups, y_true, o_x, y64, loss64, evals = _case(*key)
    B = profile[0].shape[0]
    model = model_from_params(P, cfg).train()
    # training step: loss and every parameter gradient
    model.zero_grad()
    y = model(profile=dev(profile), targets=[dev(t) for t in groups])
    y = _per_user(y, B, len(groups))
    loss = M.BinaryCrossEntropy()(y, y_true.cuda(), M.get_mask(o_x.cuda()))
    loss.backward()
    assert float((y.detach().cpu().double() - y64).abs().max()) < 2e-5
    assert abs(float(loss.detach()) - loss64) <= 2e-6 * abs(loss64), (float(loss.detach()), loss64)
    _check_params("embeds.", model.embeds, P64)
    for i, blk in enumerate(model.encoder):
        _check_params(f"encoder.{i}.", blk, P64)
    _check_params("norm.", model.norm, P64)
    _check_params("decoder.", model.decoder, P64)
    # evaluation: every user's scores, and the positive's rank where it is unambiguous
    model.eval()
    with torch.no_grad():
        for prof_e, tgt_e, want in evals:
            got = model(profile=dev(prof_e), targets=[dev(tgt_e)]).cpu()
            assert got.shape == want.shape
            assert float((got.double() - want).abs().max()) < 2e-5
            if want.dim() == 2:
                # without the decoder's residual (residual_ca=False) the empty and the one-item profile give every
                # candidate the same attention output, so all of that user's scores tie: there is no rank to compare
                ranked = (want.max(1).values - want.min(1).values) > 1e-9
                assert int(ranked.sum()) >= (B - 2 if not cfg.residual_ca else B)
                got, want = got[ranked], want[ranked]
            assert_all_users_match_oracle(got, want, 2e-5)
    assert bool(composed_calls) is expect_composed, len(composed_calls)


# (d, H, L, B, n_blocks, residual_sa, residual_ca): every geometry at least twice, exact-width and padded (d < DPI or
# dh < DHP); the comment names the kernel instance
BUILT_CASES = [
    (64, 4, 16, 7, 2, True, True),      # <64,16,4>
    (36, 4, 33, 7, 1, True, True),      # <64,16,4>   d < DPI, dh 9 of 16
    (64, 2, 64, 7, 1, True, True),      # <64,32,2>
    (48, 2, 17, 7, 1, True, True),      # <64,32,2>   dh 24 of 32
    (64, 1, 48, 7, 1, True, True),      # <64,64,1>
    (56, 1, 1, 4, 1, True, True),       # <64,64,1>   dh 56 of 64
    (96, 3, 17, 7, 1, True, True),      # <96,32,3>
    (72, 3, 64, 7, 2, False, True),     # <96,32,3>   dh 24 of 32, no residual in the blocks
    (96, 2, 1, 4, 1, True, True),       # <96,48,2>
    (80, 2, 48, 7, 1, True, True),      # <96,48,2>   dh 40 of 48
    (96, 1, 33, 7, 1, True, True),      # <96,96,1>
    (90, 1, 16, 7, 1, True, True),      # <96,96,1>   dh 90 of 96
    (128, 4, 48, 7, 1, True, True),     # <128,32,4>
    (100, 4, 16, 7, 1, True, True),     # <128,32,4>  dh 25 of 32
    (120, 4, 64, 7, 1, True, True),     # <128,32,4>  dh 30 of 32
    (128, 2, 17, 7, 1, True, True),     # <128,64,2>
    (112, 2, 64, 7, 1, True, False),    # <128,64,2>  dh 56 of 64, no residual in the decoder
    (128, 1, 64, 7, 2, True, True),     # <128,128,1>
    (120, 1, 17, 7, 1, True, True),     # <128,128,1> dh 120 of 128
]


@pytest.mark.parametrize("variant", [0, 1, 3], ids=["shared-users", "one-workgroup-per-user", "eight-wave-scoring"])
@pytest.mark.parametrize("d,H,L,B,nb,res_sa,res_ca", BUILT_CASES)
def test_built_geometry_trains_and_scores_like_the_oracle(d, H, L, B, nb, res_sa, res_ca, variant, set_variant,
                                                          composed_calls):
    from carca_replication_amd import ops

    assert ops.attn_geometry_built(d, H)
    set_variant(variant)
    _run_case((d, H, L, B, nb, res_sa, res_ca), composed_calls, expect_composed=False)


def test_built_geometry_at_160_users(composed_calls):
    """B = 160 > CUs / 2: the attention kernels give each user one workgroup by default (no tuning key set)."""
    _run_case((128, 1, 16, 160, 1, True, True, 6, 8), composed_calls, expect_composed=False)


# (d, H) the fused kernels are not built for: composed path, same checks (before routing on the built geometries these
# raised CarcaHipError "no kernel built for d=.. H=..")
UNBUILT = [(32, 2), (96, 4), (64, 8), (128, 8), (48, 1), (60, 3)]


@pytest.mark.parametrize("L", [17, 50])
@pytest.mark.parametrize("d,H", UNBUILT)
def test_unbuilt_geometry_runs_composed_like_the_oracle(d, H, L, composed_calls):
    from carca_replication_amd import ops

    assert not ops.attn_geometry_built(d, H)
    _run_case((d, H, L, 7, 1, True, True), composed_calls, expect_composed=True)


@pytest.mark.parametrize("variant", [0, 1, 3], ids=["shared-users", "one-workgroup-per-user", "eight-wave-scoring"])
def test_three_target_groups_train_like_the_oracle(variant, set_variant, composed_calls):
    """MAX_GROUPS = 3 groups in one fused training call (the most cross_attn_bwd takes), each padded differently: the
    negatives of group 2 are zeroed where the profile's first slots are, group 3 additionally on every fifth slot."""
    from carca_replication_amd import modules as M

    d, H, L, B, n_attrs = 90, 3, 33, 7, 12
    cfg = O.CarcaConfig(d=d, H=H, n_blocks=1)
    P = O.perturb_params(O.init_params(cfg, N_ITEMS, 24, N_CTX, n_attrs, L, seed=4), seed=5, scale=0.2)
    profile, _ = _batch(B, L, 1, n_attrs, 6)
    groups, _, _ = _train_targets(profile, 7, n_attrs, n_groups=3)
    g1, g2 = groups[1], groups[2]
    groups[1] = (g1[0] * (torch.arange(L) >= L // 3).int(), g1[1], g1[2])
    groups[2] = (g2[0] * (torch.arange(L) % 5 != 0).int(), g2[1], g2[2])
    p_x = profile[0]
    y_true = torch.cat([(p_x != 0).int(), torch.zeros_like(p_x), torch.zeros_like(p_x)], dim=1)
    o_x = torch.cat([g[0] for g in groups], dim=1)
    assert len({int((g[0] != 0).sum()) for g in groups}) == 3
    P64 = _P64(P)
    y64 = O.carca_forward(P64, cfg, _f64(profile), [_f64(t) for t in groups], training=True)
    loss64 = O.bce_loss(y64, y_true.double(), O.get_mask(o_x, torch.float64))
    loss64.backward()
    set_variant(variant)
    model = model_from_params(P, cfg).train()
    y = model(profile=dev(profile), targets=[dev(t) for t in groups])
    loss = M.BinaryCrossEntropy()(y, y_true.cuda(), M.get_mask(o_x.cuda()))
    loss.backward()
    assert not composed_calls
    assert float((y.detach().cpu().double() - y64.detach()).abs().max()) < 2e-5
    assert abs(float(loss.detach()) - float(loss64.detach())) <= 2e-6 * abs(float(loss64.detach()))
    _check_params("embeds.", model.embeds, P64)
    _check_params("encoder.0.", model.encoder[0], P64)
    _check_params("norm.", model.norm, P64)
    _check_params("decoder.", model.decoder, P64)
