"""The grouped hit compare of the evaluation dedup under a per-item cache (csrc/feat_dedup.hip):
the insert launch ranks the rows of each item, and the row of every fourth rank among the first LIST = 16 compares its
group with ONE read of the item's cache entry.  Tuning key 22 = 1 lets every row compare for itself, as before.

Every case runs one call sequence on two deep copies of a model, key 22 = 0 and key 22 = 1, and requires the same bits
(NaN in the same places) of q and the scores and the same counts of rows flagged and rows multiplied; q is also held
against the float64 product.  `feat_dedup_rows_grouped` is predicted on the host from the ids: the sum over the items
with a filled entry of min(rows of the item, LIST).  Which row of an item takes which rank depends on timing, so the
changed-bytes case changes every one of an item's 21 rows in turn: whatever the ranks, a first, a middle and a last row
of a group and rows past the list are among them.

Shapes: those of tests/test_hip_feat_cache.py (B = 88 is the smallest batch on the "+dedup" route; every run asserts the
route)."""
import copy

import pytest
import torch

from tests.model_util import build_model
from tests.test_hip_feat_cache import (B, CACHE_KEY, D, H, IX, IY, IZ, KN, KZ, L, N, NA, _batch, _distinct, _model, _q_ref,
                                       _run, _same, catalogue, tuning)  # noqa: F401  (two fixtures)
from tests.test_hip_feature_dedup import _close

pytestmark = pytest.mark.gpu

SOLO_KEY = 22
LIST = 16


def _ids(segs):
    ids = torch.cat([s[0].reshape(-1) for s in segs]).long()
    return ids[ids != 0]


def _grouped(segs, filled):
    """Rows a group's first row compares for: min(rows, LIST) per item of the batch whose entry is filled."""
    c = torch.bincount(_ids(segs)).tolist()
    return sum(min(c[i], LIST) for i in filled if i < len(c))


def _both(model, tuning, calls, twin=None, table_path=False, check_q=True):
    """Runs `calls` (a list of batches) on `model` with key 22 = 0 and on its deep copy with key 22 = 1; the two agree bit for
    bit.  -> per call (scores, q, rows computed, rows flagged, rows grouped) of the key-0 run."""
    from carca_replication_amd import ops

    twin = copy.deepcopy(model) if twin is None else twin
    out = []
    for value, m in ((0, model), (1, twin)):
        tuning(SOLO_KEY, value)
        res = []
        for segs in calls:
            y, q, _, computed, flagged = _run(m, segs, table_path=table_path)
            res.append((y, q, computed, flagged, ops.feat_dedup_rows_grouped()))
            if value == 0 and check_q:
                _close(q, _q_ref(m, segs))
        out.append(res)
    tuning(SOLO_KEY, 0)
    for i, (a, b) in enumerate(zip(*out)):
        assert _same(a[0], b[0]) and _same(a[1], b[1]), i
        assert a[2:4] == b[2:4], (i, a[2:], b[2:])
        assert b[4] == 0, (i, b[4])
    return out[0]


def test_heavy_repeats(catalogue, tuning):
    """About 40 rows per item: several groups per item and ranks past the list."""
    model = _model()
    warm, segs = _batch(catalogue, 21), _batch(catalogue, 22)
    filled = _distinct(warm)
    assert _distinct(segs) <= filled and int(torch.bincount(_ids(segs)).max()) > 2 * LIST
    res = _both(model, tuning, [warm, segs])
    assert res[0][2:] == (len(filled), len(filled), 0)
    assert res[1][2:] == (0, len(_distinct(segs)), _grouped(segs, filled))
    assert res[1][4] < len(_ids(segs))  # (rows past the list compared for themselves)


def test_light_repeats(tuning):
    """A catalogue of 8,000 items (a 131 MB table): one to five rows per item, every kept row in a group."""
    n_items = 8001
    gen = torch.Generator(device="cuda").manual_seed(98)
    table = torch.rand(n_items, NA, generator=gen, device="cuda")
    table[0] = 0.0
    torch.manual_seed(0)
    model = build_model(dict(d=D, H=H, n_blocks=2), n_items, 450, 6, NA, L).cuda().eval()
    segs = _batch(table, 23, lo=1, hi=n_items)
    counts = torch.bincount(_ids(segs))
    assert set(range(1, 6)) <= set(counts.tolist()) and int(counts.max()) < LIST
    n = len(_distinct(segs))
    res = _both(model, tuning, [segs, segs])
    assert res[0][2:] == (n, n, 0)
    assert res[1][2:] == (0, n, len(_ids(segs)))
    assert _same(res[1][1], res[0][1]) and _same(res[1][0], res[0][0])


def test_changed_bytes_in_one_row_of_a_group(catalogue, tuning):
    """Items IX, IY, IZ in target slots 1 .. 21 of users 0, 1, 2 and nowhere else.  Call p changes slot p (2 .. 21: never the
    item's lowest row) of each: IX's last 32-bit word one ulp up, IY's +0.0 to -0.0, IZ's NaN payload.  Those three rows
    alone are multiplied, every other row keeps the bits of the unchanged batch, and the entries keep the old bytes."""
    model = _model()
    base = _batch(catalogue, 24)
    items = (IX, IY, IZ)
    for u, it in enumerate(items):
        base[1][0][u, 1:22] = it
        base[1][1][u, 1:22] = catalogue[it]
    n = len(_distinct(base))
    up = torch.nextafter(catalogue[IX, NA - 1].cpu(), torch.tensor(2.0)).item()
    calls = [base]
    for p in range(2, 22):
        seg = tuple(t.clone() for t in base[1])
        seg[1][0, p, NA - 1] = up
        seg[1][1, p, KZ] = -0.0
        seg[1][2, p, KN] = torch.tensor(0x7FC00002, dtype=torch.int32).view(torch.float32)
        calls.append([base[0], seg])
    calls.append(base)
    res = _both(model, tuning, calls)
    want = _grouped(base, _distinct(base))
    y0, q0 = res[0][0], res[0][1]
    assert res[0][2:] == (n, n, 0)
    for p, (y, q, computed, flagged, grouped) in zip(range(2, 22), res[1:-1]):
        assert (computed, flagged, grouped) == (3, n + 3, want), p
        rows = torch.tensor([B * L + u * N + p for u in range(3)], device="cuda")
        keep = torch.ones(q.shape[0], dtype=torch.bool, device="cuda")
        keep[rows] = False
        assert _same(q[keep], q0[keep]), p
    assert res[-1][2:] == (0, n, want)
    assert _same(res[-1][1], q0) and _same(res[-1][0], y0)


def test_changed_bytes_in_the_owner_row_of_a_group(catalogue, tuning):
    """Item IX in user 0's target slots 1 .. 6; the second batch changes slot 1, the item's lowest row and the owner of its
    table slot.  The owner misses and is multiplied; the five others hit (and count as merged: flagged reads n)."""
    model = _model()
    base = _batch(catalogue, 25)
    base[1][0][0, 1:7] = IX
    base[1][1][0, 1:7] = catalogue[IX]
    n = len(_distinct(base))
    seg = tuple(t.clone() for t in base[1])
    seg[1][0, 1, NA - 1] = torch.nextafter(catalogue[IX, NA - 1].cpu(), torch.tensor(2.0)).item()
    res = _both(model, tuning, [base, [base[0], seg], base])
    want = _grouped(base, _distinct(base))
    assert res[1][2:] == (1, n, want) and res[2][2:] == (0, n, want)
    keep = torch.ones(res[0][1].shape[0], dtype=torch.bool, device="cuda")
    keep[B * L + 1] = False
    assert _same(res[1][1][keep], res[0][1][keep])
    assert _same(res[2][1], res[0][1]) and _same(res[2][0], res[0][0])


def test_partial_overlap(catalogue, tuning):
    """Filled and empty entries in one batch: the rows of an empty one compare within the batch and publish, as before."""
    model = _model()
    sa = _batch(catalogue, 26, lo=1, hi=151)
    sb = _batch(catalogue, 27, lo=76, hi=226)
    da, db = _distinct(sa), _distinct(sb)
    assert len(da & db) >= 40 and len(db - da) >= 50
    res = _both(model, tuning, [sa, sb, sb])
    assert res[1][2:] == (len(db - da), len(db), _grouped(sb, da & db))
    assert res[2][2:] == (0, len(db), _grouped(sb, db))
    assert _same(res[2][1], res[1][1])


def _off_by_one_float(t):
    """The same values in memory that starts 4 bytes past a 16-byte boundary: no 16-byte loads."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


def test_the_four_byte_compare(catalogue, tuning):
    model = _model(449, 0)
    calls = []
    for seed in (28, 29):
        segs = _batch(catalogue, seed, nc=0)
        calls.append([(x, _off_by_one_float(a), c) for x, a, c in segs])
    filled = _distinct(calls[0])
    assert _distinct(calls[1]) <= filled
    res = _both(model, tuning, calls)
    assert res[1][2:] == (0, len(_distinct(calls[1])), _grouped(calls[1], filled))


def test_one_id_everywhere(catalogue, tuning):
    model = _model()
    segs = _batch(catalogue, 30, lo=5, hi=6)
    assert _distinct(segs) == {5}
    res = _both(model, tuning, [segs, segs])
    assert res[0][2:] == (1, 1, 0) and res[1][2:] == (0, 1, LIST)
    assert _same(res[1][1], res[0][1])


def test_table_handed_back_clean(catalogue, tuning):
    """Two different batches in a row behind the one that filled the cache: per-slot counts that the expand launch left
    behind would show in the second one's groups and in its distinct rows."""
    model = _model()
    warm, sa, sb = _batch(catalogue, 31), _batch(catalogue, 32, lo=1, hi=120), _batch(catalogue, 33, lo=60, hi=297)
    filled = _distinct(warm)
    assert _distinct(sa) | _distinct(sb) <= filled
    res = _both(model, tuning, [warm, sa, sb])
    assert res[1][2:] == (0, len(_distinct(sa)), _grouped(sa, filled))
    assert res[2][2:] == (0, len(_distinct(sb)), _grouped(sb, filled))


def test_no_cache_no_groups(catalogue, tuning):
    """Key 21 = 1, a captured forward and the attribute-table path: nothing is grouped, key 22 changes nothing."""
    from carca_replication_amd import ops

    model = _model()
    segs = _batch(catalogue, 34)
    n = len(_distinct(segs))
    tuning(CACHE_KEY, 1)
    res = _both(model, tuning, [segs, segs])
    assert res[0][2:] == (n, n, 0) and res[1][2:] == (n, n, 0)
    y0, q0 = res[0][0], res[0][1]
    tuning(CACHE_KEY, 0)
    for value in (0, 1):
        tuning(SOLO_KEY, value)
        with torch.no_grad():
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                yg = model(profile=segs[0], targets=list(segs[1:]))
                zq = model.__dict__["_plan"]["zq"]  # (the captured forward's q: memory the graph owns or the plan keeps)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(yg, y0) and _same(zq[:, D:], q0)
            # (a captured launch leaves no counts: -1, and nothing grouped)
            assert (ops.feat_dedup_rows_computed(), ops.feat_dedup_rows_multiplied()) == (-1, -1)
            assert ops.feat_dedup_rows_grouped() == 0
            del graph
    tuning(SOLO_KEY, 0)
    model, twin = _model(), _model()
    model.embeds.register_attr_table(catalogue)
    twin.embeds.register_attr_table(catalogue)
    res = _both(model, tuning, [segs, segs], twin=twin, table_path=True, check_q=False)
    assert res[0][2:] == (n, n, 0) and res[1][2:] == (0, n, 0)
    assert torch.equal(res[1][0], y0)
