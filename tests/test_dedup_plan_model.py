"""The plan of the evaluation feature product over distinct attribute rows (csrc/feat_dedup.hip), restated in Python and
checked for its invariants -- no GPU needed: the id table (open addressing, 2x the rows, the lowest row of an id wins), the
byte check against the representative, the kept-row flags gemm_rows_skc_kernel plans from, and the stream-K stretches over
the representatives' row blocks.  tests/test_hip_feature_dedup.py runs the kernels themselves."""
import numpy as np
import pytest

from tests.test_skc_plan_model import pieces, split_grid


def hash_slot(i, hbits):
    return ((i * 0x9E3779B1) & 0xFFFFFFFF) >> (32 - hbits)


def plan(ids, rows, gathered=False, order=None):
    """-> rep (per row, -1 for id 0), flag (1: representative), the table left behind.  `order`: the order in which the
    rows reach the table (the GPU's is arbitrary; the result must not depend on it)."""
    R = len(ids)
    hbits = 12
    while (1 << hbits) < 2 * R:
        hbits += 1
    key = np.zeros(1 << hbits, np.int64)
    val = np.zeros(1 << hbits, np.int64)
    slot = np.full(R, -1)
    for g in (range(R) if order is None else order):  # dedup_insert_kernel
        if ids[g] == 0:
            continue
        h = hash_slot(int(ids[g]), hbits)
        while key[h] not in (0, ids[g]):
            h = (h + 1) & ((1 << hbits) - 1)
        key[h] = ids[g]
        val[h] = max(val[h], 0xFFFFFFFF - g)
        slot[g] = h
    rep, flag = np.full(R, -1), np.zeros(R, np.int32)
    owner = np.full(R, -1)
    for g in range(R):  # dedup_resolve_kernel
        if slot[g] < 0:
            continue
        r0 = 0xFFFFFFFF - val[slot[g]]
        same = r0 == g or gathered or rows[g].view(np.uint32).tobytes() == rows[r0].view(np.uint32).tobytes()
        rep[g] = r0 if (same and r0 != g) else g
        flag[g] = 0 if (same and r0 != g) else 1
        owner[g] = slot[g] if r0 == g else -1
    for g in range(R):  # dedup_expand_kernel hands the table back clean
        if owner[g] >= 0:
            key[owner[g]] = val[owner[g]] = 0
    return rep, flag, key, val


def batch(kind, R=600, K=16, seed=0):
    rng = np.random.default_rng(seed)
    ids = {"heavy": rng.integers(1, 20, R), "none": rng.permutation(R) + 1, "same": np.full(R, 5), "pad": np.zeros(R, int),
           "big": rng.integers(1, 1 << 20, R)}[kind]
    if kind not in ("pad", "same"):
        ids[rng.random(R) < 0.2] = 0
    uniq, inv = np.unique(ids, return_inverse=True)
    rows = rng.random((len(uniq), K)).astype(np.float32)[inv]
    rows[ids == 0] = 0
    return ids.astype(np.int64), rows


@pytest.mark.parametrize("kind", ["heavy", "none", "same", "pad", "big"])
def test_every_kept_row_is_covered_once_by_its_lowest_equal_row(kind):
    ids, rows = batch(kind)
    rep, flag, key, val = plan(ids, rows)
    kept = ids != 0
    assert (rep[~kept] == -1).all() and (flag[~kept] == 0).all()
    for g in np.nonzero(kept)[0]:
        u = rep[g]
        assert flag[u] == 1 and ids[u] == ids[g] and u <= g  # one representative, a multiplied row, of the same id
        assert rows[u].tobytes() == rows[g].tobytes()
        assert u == np.nonzero(ids == ids[g])[0].min()  # no byte differences here: the lowest row of the id
    assert flag.sum() == len(np.unique(ids[kept]))
    assert not key.any() and not val.any()  # the table is clean for the next batch


def test_the_groups_do_not_depend_on_the_arrival_order():
    ids, rows = batch("heavy", seed=3)
    want = plan(ids, rows)[:2]
    rng = np.random.default_rng(4)
    for _ in range(5):
        got = plan(ids, rows, order=rng.permutation(len(ids)))[:2]
        assert all((a == b).all() for a, b in zip(want, got))


@pytest.mark.parametrize("change", ["ulp", "negzero", "nan_payload"])
def test_a_byte_different_row_is_never_merged(change):
    ids, rows = batch("heavy", seed=1)
    g0, g1 = np.nonzero(ids == ids[np.nonzero(ids)[0][0]])[0][:2]
    rows[g1] = rows[g0]
    if change == "ulp":
        rows[g1, 3] = np.nextafter(rows[g0, 3], np.float32(2))
    elif change == "negzero":
        rows[[g0, g1], 3] = np.float32(0.0)
        rows[g1, 3] = np.float32(-0.0)
    else:
        rows[[g0, g1], 3] = np.array([0x7FC00001, 0x7FC00002], np.uint32).view(np.float32)
    rep, flag, _, _ = plan(ids, rows)
    assert rep[g1] == g1 and flag[g1] == 1
    # ... and the table path (one row per id) merges it: the comparison is the dense path's alone
    rep_t, _, _, _ = plan(ids, rows, gathered=True)
    assert rep_t[g1] == g0


@pytest.mark.parametrize("kind", ["heavy", "none", "big"])
@pytest.mark.parametrize("segs", [(50 * 128, 101 * 128), (50 * 128, 40 * 128, 40 * 128, 40 * 128)])
def test_the_stream_k_stretches_cover_the_representatives(kind, segs):
    """gemm_rows_skc_kernel's row blocks are 384 flagged rows of each segment; its stretches must cover every K step of
    them once per kind of workgroup (the plan of tests/test_skc_plan_model.py over the representatives' count)."""
    rng = np.random.default_rng(2)
    R = sum(segs)
    pool = {"heavy": 3000, "none": None, "big": 1 << 20}[kind]
    ids = rng.permutation(R) + 1 if pool is None else rng.integers(1, pool, R)
    ids[rng.random(R) < 0.15] = 0
    _, flag, _, _ = plan(ids, None, gathered=True)
    nrb, off = 0, 0
    for n in segs:
        nrb += (int(flag[off: off + n].sum()) + 383) // 384
        off += n
    nfast, nfull, cheap = 128, 4, 74
    total = nfast * nrb
    if nrb == 0:
        return
    x, y = split_grid(255, nfull, cheap, total)
    for nteams in (x, y):
        steps = np.zeros(total, int)
        for tj in range(nteams):
            for rb, s0, s1, _, _ in pieces(tj, nteams, total, nfast):
                steps[rb * nfast + s0: rb * nfast + s1] += 1
        assert (steps == 1).all()
