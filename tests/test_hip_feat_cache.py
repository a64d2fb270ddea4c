"""The per-item cache of the evaluation feature product (AllEmbedding.feat_cache, csrc/feat_dedup.hip):
P[i] = attrs[i] W_a^T is multiplied by the first batch that carries item i and taken from the cache afterwards, after
a byte compare of the batch row with the row the entry was computed from.

Shapes: L = 50, N = 101, d = 90, H = 3, g = 450, n_ctx = 6, n_attrs = 4096 (the stream-K kernel and the 16-byte compare)
and once g = 449, n_ctx = 0 (the 4-byte paths), ids drawn from 300 items so that every batch repeats items.  B = 88:
the product takes the "+dedup" route only on the one-block-per-CU choice of gemm_rows_choose, which at g = 450 needs
ceil(B L / 128) + ceil(B N / 128) >= 103 blocks of 128 rows -- B = 88 is the smallest batch that has them (B = 8 runs on
the narrow kernel and never meets the dedup).  Every run asserts that the route was taken."""
import copy

import pytest
import torch

from tests.model_util import build_model
from tests.test_hip_feature_dedup import _close

pytestmark = pytest.mark.gpu

D, H, NA, L, N, B = 90, 3, 4096, 50, 101, 88
NI = 301  # item ids 1 .. 300
CACHE_KEY = 21
KW, KZ, KN = 11, 12, 13  # attribute columns of the changed-bytes case: weight 1e3, a +0.0 / -0.0 element, a NaN payload
IX, IY, IZ = 297, 298, 299  # ... and its items (kept out of the random draws)


@pytest.fixture
def tuning():
    from carca_replication_amd import ops

    touched = set()

    def set_(key, value):
        touched.add(key)
        ops.set_tuning(key, value)

    yield set_
    for key in touched:
        ops.set_tuning(key, 0)


def _model(g=450, nc=6, seed=0):
    torch.manual_seed(seed)
    return build_model(dict(d=D, H=H, n_blocks=2), NI, g, nc, NA, L).cuda().eval()


@pytest.fixture(scope="module")
def catalogue():
    """The items' attribute rows [NI, NA] (row 0: padding), unchanged by every test."""
    gen = torch.Generator(device="cuda").manual_seed(99)
    t = torch.rand(NI, NA, generator=gen, device="cuda")
    t[0] = 0.0
    t[IX, KW], t[IY, KZ] = 1.0, 0.0
    t[IZ, KN] = torch.tensor(0x7FC00001, dtype=torch.int32).view(torch.float32)
    return t


def _batch(table, seed, lo=1, hi=297, nc=6, same_ctx=False):
    """(profile, target) with ids drawn from [lo, hi), left-padded profiles, a = table[x]."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    px = torch.randint(lo, hi, (B, L), generator=gen, device="cuda")
    lens = torch.randint(3, L + 1, (B,), generator=gen, device="cuda")
    px = px * (torch.arange(L, device="cuda")[None, :] >= (L - lens)[:, None])
    ox = torch.randint(lo, hi, (B, N), generator=gen, device="cuda")
    segs = []
    for x in (px, ox):
        c = torch.rand(*x.shape, nc, generator=gen, device="cuda")
        if same_ctx:
            c = torch.full((*x.shape, nc), 0.25, device="cuda")
        segs.append((x.int().contiguous(), table[x].contiguous(), c.contiguous()))
    return segs


def _distinct(segs):
    ids = torch.cat([s[0].reshape(-1) for s in segs])
    return set(torch.unique(ids[ids != 0]).tolist())


def _run(model, segs, table_path=False):
    """-> (scores, q, row-GEMM log, rows computed, rows flagged) of one eval forward."""
    from carca_replication_amd import ops

    ops.gemm_rows_log(True)
    with torch.no_grad():
        if table_path:
            y = model(profile=(segs[0][0], None, segs[0][2]), targets=[(s[0], None, s[2]) for s in segs[1:]])
        else:
            y = model(profile=segs[0], targets=list(segs[1:]))
    computed, flagged = ops.feat_dedup_rows_computed(), ops.feat_dedup_rows_multiplied()
    torch.cuda.synchronize()
    log = ops.gemm_rows_log()
    ops.gemm_rows_log(False)
    assert "+dedup" in log, log
    return y.clone(), model.__dict__["_plan"]["zq"][:, D:].clone(), log, computed, flagged


def _q_ref(model, segs):
    w = model.embeds.feats_embed.weight.double()
    b = model.embeds.feats_embed.bias.double()
    nc = segs[0][2].shape[-1]
    ids = torch.cat([s[0].reshape(-1) for s in segs])
    a = torch.cat([s[1].reshape(-1, NA) for s in segs]).double()
    q = a @ w[:, :NA].T + b
    if nc:
        q = q + torch.cat([s[2].reshape(-1, nc) for s in segs]).double() @ w[:, NA:].T
    return q * (ids != 0)[:, None].double()


def _same(a, b):
    """Equal bits wherever the values are numbers, NaN in the same places (item IZ's rows)."""
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


@pytest.mark.parametrize("g,nc", [(450, 6), (449, 0)])
def test_same_batch_twice(catalogue, g, nc):
    model = _model(g, nc)
    segs = _batch(catalogue, 1, nc=nc)
    n = len(_distinct(segs))
    y0, q0, _, computed, flagged = _run(model, segs)
    assert (computed, flagged) == (n, n)
    _close(q0, _q_ref(model, segs))
    y1, q1, _, computed, flagged = _run(model, segs)
    assert (computed, flagged) == (0, n)
    assert torch.equal(q1, q0) and torch.equal(y1, y0)


def test_partial_overlap(catalogue):
    model = _model()
    sa = _batch(catalogue, 2, lo=1, hi=151, same_ctx=True)
    sb = _batch(catalogue, 3, lo=76, hi=226, same_ctx=True)
    da, db = _distinct(sa), _distinct(sb)
    assert 40 <= len(da & db) <= 75 and len(db - da) >= 50
    _, qa, _, computed, _ = _run(model, sa)
    assert computed == len(da)
    _, qb, _, computed, flagged = _run(model, sb)
    assert computed == len(db - da) and flagged == len(db)
    _close(qb, _q_ref(model, sb))
    # rows of an id both batches carry, under the same context: A's bits
    ida = torch.cat([s[0].reshape(-1) for s in sa]).long()
    idb = torch.cat([s[0].reshape(-1) for s in sb]).long()
    first_a = torch.full((NI,), -1, dtype=torch.long, device="cuda")
    first_a.scatter_reduce_(0, ida, torch.arange(len(ida), device="cuda"), reduce="amax")
    shared = (idb != 0) & (first_a[idb] >= 0)
    assert int(shared.sum()) > 1000
    assert torch.equal(qb[shared], qa[first_a[idb[shared]]])


def test_changed_bytes_under_a_cached_id(catalogue):
    """Items IX, IY, IZ twice each in user 0's target slots 1 .. 6; the second batch changes the later row of each pair: one
    element one ulp up (its column weighs 1e3, so a row served from the cache would repeat the base row's q bit for bit),
    +0.0 -> -0.0, another NaN payload.  Each changed row is multiplied in its batch, the entry keeps the old bytes."""
    model = _model()
    with torch.no_grad():
        model.embeds.feats_embed.weight[:, KW] = 1e3
    base = _batch(catalogue, 4)
    base[1][0][0, 1:7] = torch.tensor([IX, IX, IY, IY, IZ, IZ], dtype=torch.int32, device="cuda")
    base[1][1][0, 1:7] = catalogue[base[1][0][0, 1:7].long()]
    n = len(_distinct(base))
    y0, q0, _, computed, _ = _run(model, base)
    assert computed == n
    changed = [base[0], tuple(t.clone() for t in base[1])]
    a = changed[1][1]
    a[0, 2, KW] = torch.nextafter(torch.tensor(1.0), torch.tensor(2.0)).item()
    a[0, 4, KZ] = -0.0
    a[0, 6, KN] = torch.tensor(0x7FC00002, dtype=torch.int32).view(torch.float32)
    _, q1, _, computed, flagged = _run(model, changed)
    assert (computed, flagged) == (3, n + 3)
    r = lambda s: B * L + s  # noqa: E731  (user 0's target slot s)
    _close(q1, _q_ref(model, changed))
    assert not torch.equal(q1[r(2)], q1[r(1)])
    assert _same(q1[r(1)], q0[r(1)]) and _same(q1[r(3)], q0[r(3)])
    assert bool(torch.isnan(q1[r(5)]).all()) and bool(torch.isnan(q1[r(6)]).all())
    y2, q2, _, computed, flagged = _run(model, base)
    assert (computed, flagged) == (0, n)
    assert _same(q2, q0) and _same(y2, y0)


def test_changed_bytes_in_the_owner_row(catalogue):
    """Item IX in user 0's target slots 1 and 2, nowhere else; the second batch changes slot 1, the id's LOWEST row and so
    the owner of its table slot: the owner misses and is multiplied again while slot 2 still hits and reads the cache.
    Both rows come out right, the entry keeps the old bytes.  (The hit row does not own the slot and counts as merged:
    the flagged rows read n, not n + 1 -- the edge include/carca_hip.h documents.)"""
    model = _model()
    with torch.no_grad():
        model.embeds.feats_embed.weight[:, KW] = 1e3
    base = _batch(catalogue, 9)
    base[1][0][0, 1:3] = IX
    base[1][1][0, 1:3] = catalogue[IX]
    n = len(_distinct(base))
    _, q0, _, computed, _ = _run(model, base)
    assert computed == n
    changed = [base[0], tuple(t.clone() for t in base[1])]
    changed[1][1][0, 1, KW] = torch.nextafter(torch.tensor(1.0), torch.tensor(2.0)).item()
    _, q1, _, computed, flagged = _run(model, changed)
    assert (computed, flagged) == (1, n)
    r = lambda s: B * L + s  # noqa: E731
    _close(q1, _q_ref(model, changed))
    assert torch.equal(q1[r(2)], q0[r(2)]) and not torch.equal(q1[r(1)], q0[r(1)])
    _, q2, _, computed, _ = _run(model, base)
    assert computed == 0 and torch.equal(q2, q0)


def test_dense_batches_with_a_table_registered(catalogue):
    """A registered attribute table does not decide the path: a batch that brings its rows is compared by bytes."""
    model = _model()
    model.embeds.register_attr_table(catalogue)
    segs = _batch(catalogue, 16)
    n = len(_distinct(segs))
    y0, _, _, computed, _ = _run(model, segs)
    assert computed == n
    y1, _, _, computed, _ = _run(model, segs)
    assert computed == 0 and torch.equal(y1, y0)
    y2, _, _, computed, _ = _run(model, segs, table_path=True)  # (another source of rows: every entry empty again)
    assert computed == n and torch.equal(y2, y0)


@pytest.mark.parametrize("how", ["in_place", "training_forward"])
def test_weight_changes_empty_the_cache(catalogue, how):
    model = _model()
    segs = _batch(catalogue, 5)
    n = len(_distinct(segs))
    assert _run(model, segs)[3] == n
    assert _run(model, segs)[3] == 0
    if how == "in_place":
        with torch.no_grad():
            model.embeds.feats_embed.weight.mul_(0.5)
    else:
        model.train()
        model(profile=segs[0], targets=list(segs[1:]))
        model.eval()
    _, q, _, computed, _ = _run(model, segs)
    assert computed == n
    _close(q, _q_ref(model, segs))


def test_table_path(catalogue):
    model = _model()
    segs = _batch(catalogue, 6)
    n = len(_distinct(segs))
    y_dense = _run(model, segs)[0]
    model.embeds.register_attr_table(catalogue)
    y0, _, _, computed, _ = _run(model, segs, table_path=True)
    assert computed == n  # (another source of rows: every entry empty again)
    y1, _, _, computed, flagged = _run(model, segs, table_path=True)
    assert (computed, flagged) == (0, n)
    assert torch.equal(y0, y_dense) and torch.equal(y1, y_dense)
    assert model.embeds.__dict__["_feat_cache"]["A"] is not None  # (the dense call's; the table path reads none)
    model.embeds.register_attr_table(catalogue.clone())
    y2, _, _, computed, _ = _run(model, segs, table_path=True)
    assert computed == n and torch.equal(y2, y_dense)


def test_side_stream_and_graph_bypass_the_cache(catalogue):
    from carca_replication_amd import ops

    model = _model()
    segs = _batch(catalogue, 7)
    n = len(_distinct(segs))
    y0, _, _, computed, _ = _run(model, segs)
    assert computed == n
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ys = model(profile=segs[0], targets=list(segs[1:]))
            assert ops.feat_dedup_rows_computed() == n
        torch.cuda.current_stream().wait_stream(side)
        assert torch.equal(ys, y0)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            yg = model(profile=segs[0], targets=list(segs[1:]))
        for _ in range(3):
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(yg, y0)
        del graph
    y1, _, _, computed, _ = _run(model, segs)
    assert computed == 0 and torch.equal(y1, y0)


@pytest.mark.parametrize("how", ["switch", "budget"])
def test_switch_and_budget(catalogue, tuning, monkeypatch, how):
    from carca_replication_amd import modules as M

    model = _model()
    twin = copy.deepcopy(model)
    segs = _batch(catalogue, 8)
    n = len(_distinct(segs))
    y_on, _, log_on, _, _ = _run(model, segs)  # (a cold call: every launch computes what the parent's does)
    if how == "switch":
        tuning(CACHE_KEY, 1)
    else:
        monkeypatch.setattr(M, "FEAT_CACHE_BUDGET", M.feat_cache_bytes(NI, NA, 450) - 1)
    for _ in range(2):
        y, _, log, computed, flagged = _run(twin, segs)
        assert (computed, flagged) == (n, n)
        assert "_feat_cache" not in twin.embeds.__dict__
        # (the same launches from the dedup on: the first model's log starts with its one-time z_table product)
        assert log[log.index("gemm_rows_skc"):] == log_on[log_on.index("gemm_rows_skc"):] and torch.equal(y, y_on)


def test_a_sequence_of_batches_against_the_switch_off(catalogue, tuning):
    model = _model()
    twin = copy.deepcopy(model)
    batches = [_batch(catalogue, 10 + i) for i in range(4)]
    on = [_run(model, s) for s in batches]
    assert on[3][3] < on[0][3]
    tuning(CACHE_KEY, 1)
    off = [_run(twin, s) for s in batches]
    for (y1, *_), (y0, *_) in zip(on, off):
        diff = float((y1 - y0).abs().max())
        assert diff <= 1e-5 * (1.0 + float(y0.abs().max())), diff
        # the positive's rank among its candidates, except where two scores are within the difference of the two runs
        gap = (y0 - y0[:, :1]).abs()
        tie = (gap <= 2 * diff).sum(1) > 1
        r1 = (y1 > y1[:, :1]).sum(1)
        r0 = (y0 > y0[:, :1]).sum(1)
        assert torch.equal(r1[~tie], r0[~tie])
