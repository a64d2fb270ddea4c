"""CARCA.recommend_users, catalogue.AudienceTopK and train.audience (carca_recommend_users / carca_audience_read; DESIGN.md
section 24) on the GPU.  The reference is S = model.score_items(prof, ctx, ids.expand(B, Q)) -- the scores existing tests
pin to the fp64 oracle -- with an eligibility mask from the exclusion sets: values and users of every row against
torch.topk over the user axis of S, exact order wherever the reference's scores are distinct, the tie rule on duplicated
rows, and bit-identity across splits of the users into updates."""
import numpy as np
import pytest
import torch

from carca_replication_amd import CarcaHipError
from carca_replication_amd.catalogue import AudienceTopK, CandidateSet
from tests.test_hip_candidates import MODELS, _draw, _model
from tests.test_hip_recommend import _excl_sets, _setup

pytestmark = pytest.mark.gpu

CHUNK = 64  # users the merge kernel takes per round (csrc/recommend_users.hip: AU_ROWS)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _scores(model, prof, ctx, ids, **kw):
    """S [B, Q] on the CPU: score_items over the listed ids for every user."""
    B = prof[0].shape[0]
    return model.score_items(prof, ctx, ids.view(1, -1).expand(B, -1).contiguous().cuda(), **kw).cpu()


def _eligible(p_x, ids, exclude, user_ids=None):
    """[B, Q] bool on the CPU: user b may be named for item ids[q]."""
    B = p_x.shape[0]
    if isinstance(exclude, str):
        sets = _excl_sets(p_x)
    elif exclude is None:
        sets = [set() for _ in range(B)]
    else:
        sets = _excl_sets(torch.zeros_like(p_x), exclude.cpu())
    el = torch.tensor([[int(i) not in sets[b] for i in ids.tolist()] for b in range(B)], dtype=torch.bool).view(B, ids.numel())
    if user_ids is not None:
        el &= (user_ids.cpu() >= 0).view(B, 1)
    return el


def _check(got, S, el, ids, k, user_ids=None, tied_on_purpose=False):
    """Values, users and, where the reference's top k + 1 scores are distinct, the exact order of every row; the share of
    columns left out of the exact check is capped at 10 %.  tied_on_purpose: the batch repeats rows, so most columns tie
    and the caller checks the order of the tied users itself; values and users are checked as always."""
    scores, users, item_ids = (t.cpu() for t in got)
    B, Q = el.shape
    assert scores.dtype == torch.float32 and users.dtype == torch.int64 and item_ids.dtype == torch.int64
    assert tuple(scores.shape) == (Q, k) and tuple(users.shape) == (Q, k)
    assert torch.equal(item_ids, ids.to(torch.int64))
    uid = list(range(B)) if user_ids is None else user_ids.cpu().tolist()
    inexact = 0
    for q in range(Q):
        rows = torch.nonzero(el[:, q]).view(-1)
        col = S[rows, q]
        m = min(k, rows.numel())
        assert not bool(scores[q, m:].any()) and bool((users[q, m:] == -1).all())  # padding: exactly 0 / -1
        if m == 0:
            continue
        top = torch.topk(col, min(k + 1, rows.numel()))
        assert torch.equal(_bits(scores[q, :m]), _bits(top.values[:m]))
        got_u = users[q, :m].tolist()
        row_of = {uid[b]: b for b in rows.tolist()}
        assert len(set(got_u)) == m and set(got_u) <= set(row_of)  # distinct and eligible
        mine = torch.stack([S[row_of[u], q] for u in got_u])
        assert torch.equal(_bits(mine), _bits(scores[q, :m]))
        if torch.unique(top.values).numel() == top.values.numel():
            assert got_u == [uid[int(rows[i])] for i in top.indices[:m].tolist()], q
        else:
            inexact += 1
    if not tied_on_purpose:
        assert inexact <= 0.10 * Q, (inexact, Q)  # the exact check must cover at least 90 % of the columns


def _ids(n, Q, seed=3):
    return torch.sort(_draw(n, Q, seed)).values if Q else torch.zeros(0, dtype=torch.int64)


# ---- values, users, exact order over the shapes -------------------------------------------------------------------------
SHAPES = [(300, 1), (300, 5), (4097, CHUNK + 1), (300, 3 * CHUNK + 5)]  # (the last: several rounds behind a threshold)


@pytest.mark.parametrize("n,B", SHAPES, ids=[f"n{n}-B{B}" for n, B in SHAPES])
@pytest.mark.parametrize("name", list(MODELS))
def test_rows_match_topk_over_the_user_axis(name, n, B):
    model, prof, ctx, p_x = _model(name, n, B)
    for Q, ks in ((0, (10,)), (1, (1, 10)), (15, (10,)), (16, (10, 128)), (17, (1, 10)), (257, (10, 128))):
        ids = _ids(n, Q)
        S = _scores(model, prof, ctx, ids) if Q else torch.zeros(B, 0)
        el = _eligible(p_x, ids, "profile")
        for k in ks:  # k = 10 and 128 exceed B = 1 and 5, and 128 exceeds B = 65: rows end in padding
            got = model.recommend_users(prof, ctx, ids.cuda(), k=k)
            _check(got, S, el, ids, k)


def test_a_set_and_a_mask_give_what_the_raw_list_gives():
    n = 300
    model, prof, ctx, p_x = _model("ca", n)
    raw = torch.tensor([40, 7, 7, 0, 299, n + 5, 12])  # unsorted, a repeat, id 0 and an id outside the catalogue
    want = model.recommend_users(prof, ctx, raw.cuda(), k=3)
    assert want[2].tolist() == [7, 12, 40, 299]
    mask = torch.zeros(n, dtype=torch.bool)
    mask[[0, 7, 12, 40, 299]] = True
    for items in (CandidateSet(raw, n, device="cuda"), CandidateSet(raw, n), mask.cuda()):
        got = model.recommend_users(prof, ctx, items, k=3)
        assert all(torch.equal(a, b) for a, b in zip(got, want))


# ---- exclusion forms, a column nobody is eligible for, dropped rows ----------------------------------------------------
@pytest.mark.parametrize("name", list(MODELS))
def test_exclusion_forms_and_negative_user_ids(name):
    n, B, Q, k = 300, 5, 17, 4
    model, prof, ctx, p_x = _model(name, n, B)
    ids = _ids(n, Q)
    S = _scores(model, prof, ctx, ids)
    rng = np.random.default_rng(9)
    lst = torch.from_numpy(rng.choice(ids.numpy(), size=(B, 6)))
    lst[:, 0] = ids[2]  # every user excludes item ids[2]: that row is all padding
    lst[:, 1] = 0       # (0 = no entry)
    lst[0, 2], lst[1, 3] = n + 9, -4  # ids outside the catalogue are ignored
    for exclude in ("profile", None, lst.cuda(), lst.to(torch.int32).cuda()):
        got = model.recommend_users(prof, ctx, ids.cuda(), k=k, exclude=exclude)
        _check(got, S, _eligible(p_x, ids, exclude), ids, k)
    got = model.recommend_users(prof, ctx, ids.cuda(), k=k, exclude=lst.cuda())
    assert not bool(got[0][2].any()) and bool((got[1][2] == -1).all())
    assert int((got[1] >= 0).sum()) > Q  # (and the other rows do name users)
    # explicit ids, two rows dropped by a negative one; int32 and int64 alike
    uids = torch.tensor([30, -1, 7, -(1 << 40), 2])
    want = model.recommend_users(prof, ctx, ids.cuda(), k=k, exclude=None, user_ids=uids.cuda())
    _check(want, S, _eligible(p_x, ids, None, uids), ids, k, uids)
    assert set(want[1].cpu().view(-1).tolist()) == {30, 7, 2, -1}
    got = model.recommend_users(prof, ctx, ids.cuda(), k=k, exclude=None, user_ids=uids.clamp(min=-1).to(torch.int32).cuda())
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    every = model.recommend_users(prof, ctx, ids.cuda(), k=k, exclude=None, user_ids=torch.full((B,), -1).cuda())
    assert not bool(every[0].any()) and bool((every[1] == -1).all())


# ---- the tie rule --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MODELS))
def test_ties_go_to_the_smaller_user_id(name):
    n, B, Q = 300, 5, 17
    model, prof, ctx, p_x = _model(name, n, B)
    p_x, p_c, ctx = p_x.clone(), prof[2].clone(), ctx.clone()
    for dup in (1, 3):  # rows 1 and 3 repeat row 0: the same logit bits for every item
        p_x[dup], p_c[dup], ctx[dup] = p_x[0], p_c[0], ctx[0]
    prof = (p_x.cuda(), None, p_c)
    ids = _ids(n, Q)
    S = _scores(model, prof, ctx, ids)
    assert torch.equal(_bits(S[0]), _bits(S[1])) and torch.equal(_bits(S[0]), _bits(S[3]))
    users = model.recommend_users(prof, ctx, ids.cuda(), k=B, exclude=None)[1].cpu()
    down = torch.tensor([40, 30, 20, 10, 0])  # descending ids: rows 0, 1, 3 are users 40, 30, 10
    named = model.recommend_users(prof, ctx, ids.cuda(), k=B, exclude=None, user_ids=down.cuda())[1].cpu()
    for q in range(Q):
        at = [users[q].tolist().index(u) for u in (0, 1, 3)]
        assert at[1] == at[0] + 1 and at[2] == at[1] + 1, q  # side by side, the smaller id first
        at = [named[q].tolist().index(u) for u in (10, 30, 40)]
        assert at[1] == at[0] + 1 and at[2] == at[1] + 1, q
    # a list shorter than the tie keeps its smallest ids
    el = _eligible(p_x, ids, None)
    short = model.recommend_users(prof, ctx, ids.cuda(), k=2, exclude=None)
    _check(short, S, el, ids, 2, tied_on_purpose=True)
    for row in short[1].cpu().tolist():
        assert 3 not in row and (1 not in row or row == [0, 1]), row
    first = model.recommend_users(prof, ctx, ids.cuda(), k=1, exclude=None)[1].cpu().view(-1)
    assert not bool(((first == 1) | (first == 3)).any())


# ---- a profile past 64 slots ----------------------------------------------------------------------------------------------
def test_a_profile_of_65_slots_with_allow_composed():
    from tests.test_hip_recommend_long import _profiles

    d, H, L, n, n_ctx, B, k, Q = 64, 4, 65, 300, 6, 5, 3, 17
    _, _, _, batch, model = _setup(d, H, "attrctx", "ca", "learnable", False, L, B, n, n_ctx, 1)
    p_x, p_c = _profiles(B, L, n, n_ctx, [0, 1, 64, 65, 65], seed=11)
    prof, ctx = (p_x.cuda(), None, p_c.float().cuda()), batch[2].float().cuda()
    ids = _ids(n, Q)
    with pytest.raises(CarcaHipError, match="64"):
        model.recommend_users(prof, ctx, ids.cuda(), k=k)
    S = _scores(model, prof, ctx, ids, allow_composed=True)
    got = model.recommend_users(prof, ctx, ids.cuda(), k=k, allow_composed=True)
    _check(got, S, _eligible(p_x, ids, "profile"), ids, k)


# ---- split invariance ------------------------------------------------------------------------------------------------------
def _cut(prof, ctx, a, b):
    return (prof[0][a:b], None, prof[2][a:b]), ctx[a:b]


@pytest.mark.parametrize("k", [10, 128])
@pytest.mark.parametrize("name", list(MODELS))
def test_the_state_does_not_depend_on_how_users_are_split(name, k):
    n, B, Q = 4097, CHUNK + 1, 17
    model, prof, ctx, p_x = _model(name, n, B)
    ids = _ids(n, Q)
    whole = AudienceTopK(ids, k, n, device="cuda")
    whole.update(model, prof, ctx)
    assert whole.rows_seen == B
    want = whole.result()
    _check(want, _scores(model, prof, ctx, ids), _eligible(p_x, ids, "profile"), ids, k)
    bounds = [(0, 1), (1, 21), (21, 28), (28, 28 + 37)]  # uneven updates, one of a single user
    assert bounds[-1][1] == B
    parts = AudienceTopK(CandidateSet(ids, n, device="cuda"), k, n)
    for a, b in bounds:  # (user_ids=None: the ids continue from the rows seen so far)
        parts.update(model, *_cut(prof, ctx, a, b))
    back = AudienceTopK(ids, k, n, device="cuda")
    for a, b in bounds[::-1]:
        back.update(model, *_cut(prof, ctx, a, b), user_ids=torch.arange(a, b).cuda())
    for st in (parts, back):
        assert st.rows_seen == B and torch.equal(st.keys, whole.keys)
        assert all(torch.equal(x, y) for x, y in zip(st.result(), want))
    flipped = whole.keys ^ (-(1 << 63))  # rows stay sorted descending as unsigned keys, empty entries last
    assert bool((flipped[:, 1:] <= flipped[:, :-1]).all())
    whole.reset()
    assert not bool(whole.keys.any()) and whole.rows_seen == 0
    s, u, _ = whole.result()
    assert not bool(s.any()) and bool((u == -1).all())


def test_recommend_users_is_one_update_of_a_fresh_state():
    n, B, Q, k = 300, 5, 15, 10
    for name in MODELS:
        model, prof, ctx, _ = _model(name, n, B)
        ids = _ids(n, Q)
        a = model.recommend_users(prof, ctx, ids.cuda(), k=k)
        b = model.recommend_users(prof, ctx, ids.cuda(), k=k)
        st = AudienceTopK(ids, k, n, device="cuda")
        st.update(model, prof, ctx)
        for other in (b, st.result()):
            assert all(torch.equal(x, y) for x, y in zip(a, other))


# ---- a row against recommend ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MODELS))
def test_scores_are_recommends_for_the_same_pair(name):
    n, B, Q, k = 300, 5, 3, 5
    model, prof, ctx, _ = _model(name, n, B)
    ids = _ids(n, Q, seed=8)
    scores, users, item_ids = (t.cpu() for t in model.recommend_users(prof, ctx, ids.cuda(), k=k, exclude=None))
    assert int((users >= 0).sum()) == Q * k
    for q in range(Q):
        for j in range(k):
            u = int(users[q, j])
            one, ctx1 = _cut(prof, ctx, u, u + 1)
            s, i = model.recommend(one, ctx1, k=1, exclude=None, candidates=item_ids[q:q + 1].cuda())
            assert int(i) == int(item_ids[q]) and torch.equal(_bits(s.cpu().view(1)), _bits(scores[q, j].view(1)))


# ---- train.audience ------------------------------------------------------------------------------------------------------
def test_audience_walks_a_loader():
    from carca_replication_amd.device_data import DeviceInteractions, DeviceLoader
    from carca_replication_amd.train import audience
    from tests.test_hip_recommend import _log

    n_items, n_ctx, L, k = 200, 6, 16, 5
    _, _, _, _, model = _setup(64, 2, "all", "ca", "identity", True, L, 2, n_items, n_ctx, 1)
    profiles, ctxd = _log(24, n_items, n_ctx, 3)
    log = DeviceInteractions(profiles, ctxd, n_items)
    items = torch.tensor([150, 3, 77, 3, 42])
    loader = DeviceLoader(log, "test", batch_size=8, profile_seq_len=L, target_seq_len=10)
    got = audience(model, loader, "cuda", items, k=k)
    st, seen = AudienceTopK(items, k, n_items, device="cuda"), 0
    for p_x, p_a, p_c, _o_x, _o_a, o_c, _y in loader:
        st.update(model, (p_x, p_a, p_c), o_c[:, 0], user_ids=torch.arange(seen, seen + p_x.shape[0]).cuda())
        seen += p_x.shape[0]
    assert seen == 24 and got[2].tolist() == [3, 42, 77, 150]
    assert all(torch.equal(a, b) for a, b in zip(got, st.result()))
    assert int((got[1] >= 0).sum()) == 4 * k and int(got[1].max()) >= 8  # (users beyond the first batch are named)
    other = audience(model, DeviceLoader(log, "test", batch_size=5, profile_seq_len=L, target_seq_len=10), "cuda",
                     CandidateSet(items, n_items), k=k)
    assert all(torch.equal(a, b) for a, b in zip(got, other))  # the loader's batch size does not show
