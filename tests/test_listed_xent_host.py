"""Host-side pieces of the softmax over per-list negatives, on the CPU: catalogue.NegativeLists
against a plain Python loop, ops.listed_xent_plan's bound, sampling.HardNegativeMiner's list assembly over a stub model,
and the fp64 reference's identities with the references of sections 13 and 14."""
import math
from types import SimpleNamespace

import pytest
import torch

from carca_replication_amd import CarcaHipError, ops
from carca_replication_amd.catalogue import NegativeLists
from carca_replication_amd.sampling import HardNegativeMiner
from tests.listed_xent_ref import list_index, ref_loss


def _csr_by_loop(lists, n_items):
    """(off, ent): per distinct live id ascending, the flat positions g N + j of its entries ascending."""
    flat = [int(x) for x in lists.reshape(-1).tolist()]
    ids = sorted({x for x in flat if 1 <= x < n_items})
    off, ent = [0], []
    for i in ids:
        ent += [e for e, x in enumerate(flat) if x == i]
        off.append(len(ent))
    return off, ent


def _check_lists(lists, n_items):
    nl = NegativeLists(lists, n_items)
    ids, index = list_index(lists, n_items)
    off, ent = _csr_by_loop(lists, n_items)
    U = ids.numel()
    assert len(nl) == U and nl.G == lists.shape[0] and nl.N == lists.shape[1] and nl.n_items == n_items
    for t in (nl.ids, nl.index, nl.lists, nl.csr_off, nl.csr_ent):
        assert t.dtype == torch.int32 and t.is_contiguous()
    assert nl.ids.tolist() == ids.tolist()
    assert nl.index.tolist() == index.tolist()
    assert nl.csr_off.tolist() == off
    assert nl.csr_ent[: off[-1]].tolist() == ent  # (past csr_off[U]: the padding entries, never read)
    assert nl.csr_ent.numel() == lists.numel()
    live = (lists >= 1) & (lists < n_items)
    assert torch.equal(nl.lists.long()[live], lists.long()[live])
    assert not bool(((nl.lists >= 1) & (nl.lists < n_items))[~live].any())
    return nl


def test_negative_lists_match_a_python_loop():
    g = torch.Generator().manual_seed(0)
    lists = torch.randint(-2, 14, (7, 9), generator=g)  # duplicates inside and across lists; 0, negatives, >= n_items
    lists[3] = torch.tensor([0, -1, 12, 13, 0, 0, -5, 12, 40])  # an all-padding list
    lists[4, :4] = 5
    _check_lists(lists, 12)
    _check_lists(torch.randint(1, 500, (3, 200), generator=g), 500)
    _check_lists(torch.tensor([[3]]), 4)
    _check_lists(torch.randint(0, 2 ** 40, (2, 5), generator=g), 100)  # (no int64 id wraps into range)


def test_negative_lists_all_padding_has_no_items():
    nl = _check_lists(torch.tensor([[0, -1, 9], [10, 0, 0]]), 9)
    assert len(nl) == 0 and nl.ids.numel() == 0 and nl.csr_off.tolist() == [0]
    assert bool((nl.index == -1).all())


def test_negative_lists_bias_and_errors():
    lists = torch.tensor([[1, 2], [2, 3]])
    nl = NegativeLists(lists, 5, bias=torch.tensor([[0.5, 1.0], [0.0, -1.0]], dtype=torch.float64))
    assert nl.bias.dtype == torch.float32 and nl.bias.tolist() == [[0.5, 1.0], [0.0, -1.0]]
    assert nl.to("cpu") is nl
    with pytest.raises(CarcaHipError, match="bias"):
        NegativeLists(lists, 5, bias=torch.zeros(2, 3))
    with pytest.raises(CarcaHipError, match="integer tensor"):
        NegativeLists(lists.float(), 5)
    with pytest.raises(CarcaHipError, match="integer tensor"):
        NegativeLists(lists.reshape(-1), 5)
    with pytest.raises(CarcaHipError, match="n_items"):
        NegativeLists(lists, 0)
    with pytest.raises(CarcaHipError, match="2\\^31"):
        NegativeLists(torch.zeros(1, 1, dtype=torch.int8).expand(2 ** 16, 2 ** 15), 5)  # (a view: no 2 GiB of ids)


@pytest.mark.parametrize("G,rpl,N,U,d,n_cus", [(1, 1, 1, 1, 64, 256), (128, 50, 4096, 300000, 128, 256), (128, 50, 128, 9000, 90, 256),
                                                (6400, 1, 1024, 100, 90, 256), (3, 1024, 5000, 0, 256, 304), (300, 3, 17, 40, 7, 1)])
def test_plan_bound(G, rpl, N, U, d, n_cus):
    plan = ops.listed_xent_plan(G, rpl, N, U, d, n_cus)
    R, ld = G * rpl, (d + 3) // 4 * 4
    assert 1 <= plan["splits"] <= 256 and plan["entries_per_split"] % 64 == 0
    assert plan["splits"] * plan["entries_per_split"] >= N > (plan["splits"] - 1) * plan["entries_per_split"]
    # the one large buffer is the [G N, ld] entry partials; beside it the dP partials and O(R) words of lists
    assert plan["scratch_bwd"] <= (G * N + (plan["splits"] + 1) * R) * ld + 4 * R + 512
    assert plan["scratch_fwd"] <= 2 * plan["splits"] * R + 4 * R + 512
    for bad in ((0, 1, 1, 1, 8), (1, 0, 1, 1, 8), (1, 1025, 1, 1, 8), (1, 1, 0, 1, 8), (1, 1, 1, -1, 8), (1, 1, 1, 1, 0),
                (2 ** 16, 1, 2 ** 15, 1, 8)):
        with pytest.raises(CarcaHipError):
            ops.listed_xent_plan(*bad)


class _Stub(torch.nn.Module):
    """A model whose retrieve returns the first k columns of a fixed [B, 12] tensor (or raises)."""

    def __init__(self, n_items, ids, fail=False):
        super().__init__()
        self.embeds = SimpleNamespace(items_embed=SimpleNamespace(num_embeddings=n_items))
        self.ids, self.fail, self.calls = ids, fail, []

    def retrieve(self, profile, context, k=1000, exclude="profile"):
        self.calls.append(dict(context=context, k=k, exclude=exclude, training=self.training,
                               grad=torch.is_grad_enabled()))
        if self.fail:
            raise RuntimeError("retrieve failed")
        return torch.zeros(self.ids.shape[0], k), self.ids[:, :k]


def test_miner_assembles_the_lists():
    n_items, B, L = 50, 3, 4
    ids = torch.arange(1, 37).reshape(B, 12)
    p_x = torch.tensor([[0, 0, 5, 6], [1, 2, 3, 4], [0, 0, 0, 9]])
    pos = torch.tensor([[0, 0, 6, 7], [2, 3, 4, 8], [0, 0, 0, 10]])
    model = _Stub(n_items, ids).train()
    torch.manual_seed(0)
    nl = HardNegativeMiner(n_hard=5, n_uniform=3, skip_top=2).mine(model, (p_x, None, torch.zeros(B, L, 2)), pos)
    assert isinstance(nl, NegativeLists) and (nl.G, nl.N, nl.n_items) == (B, 8, n_items)
    assert nl.lists.dtype == torch.int32
    assert torch.equal(nl.lists[:, :5].long(), ids[:, 2:7])  # columns skip_top onwards
    tail = nl.lists[:, 5:]
    assert bool(((tail >= 1) & (tail < n_items)).all())  # the uniform tail
    (call,) = model.calls
    assert call["context"] is None and call["k"] == 7 and not call["training"] and not call["grad"]
    assert torch.equal(call["exclude"], torch.cat([p_x, pos], 1))
    assert model.training  # (the previous mode is back)
    model.eval()
    nl = HardNegativeMiner(n_hard=4).mine(model, (p_x, None, torch.zeros(B, L, 2)), pos)
    assert (nl.G, nl.N) == (B, 4) and torch.equal(nl.lists.long(), ids[:, :4]) and not model.training
    nl = HardNegativeMiner(n_hard=0, n_uniform=6).mine(model, (p_x, None, torch.zeros(B, L, 2)), pos)
    assert (nl.G, nl.N) == (B, 6) and len(model.calls) == 2  # (no retrieve without a hard part)
    with pytest.raises(ValueError):
        HardNegativeMiner(n_hard=0, n_uniform=0)
    with pytest.raises(ValueError):
        HardNegativeMiner(n_hard=3, skip_top=-1)


def test_miner_restores_the_mode_when_retrieve_raises():
    model = _Stub(50, torch.zeros(2, 12, dtype=torch.int64), fail=True).train()
    p_x = torch.ones(2, 3, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="retrieve failed"):
        HardNegativeMiner(n_hard=5).mine(model, (p_x, None, torch.zeros(2, 3, 1)), p_x)
    assert model.training and torch.is_grad_enabled()


def _rows(R, d, n_items, seed):
    g = torch.Generator().manual_seed(seed)
    P = torch.randn(R, d, generator=g, dtype=torch.float64)
    table = torch.randn(n_items, d, generator=g, dtype=torch.float64) / d ** 0.5
    pos = torch.randint(1, n_items, (R,), generator=g)
    pos[torch.rand(R, generator=g) < 0.2] = 0
    pos[0], pos[1] = n_items + 2, -1
    return P, table, pos


def test_reference_with_full_lists_is_the_catalogue_reference():
    from tests.test_hip_catalogue_xent import _ref_loss as catalogue_ref

    n_items, d, G, rpl = 40, 8, 5, 6
    P, table, pos = _rows(G * rpl, d, n_items, 1)
    lists = torch.arange(1, n_items).view(1, -1).expand(G, n_items - 1)
    ids, index = list_index(lists, n_items)
    got = ref_loss(P, table[pos.clamp(0, n_items - 1)], pos, table[ids], lists, index, rpl, n_items)
    want = catalogue_ref(P, table, pos)
    assert abs(got.item() - want.item()) <= 1e-12 * abs(want.item())


def test_reference_with_one_shared_list_is_the_sampled_reference():
    from tests.test_hip_sampled_xent import _ref_loss as sampled_ref

    n_items, d, G, rpl, K = 40, 8, 5, 6, 30
    P, table, pos = _rows(G * rpl, d, n_items, 2)
    g = torch.Generator().manual_seed(3)
    s = torch.randint(1, n_items, (K,), generator=g)
    s[:8] = pos[torch.randint(0, G * rpl, (8,), generator=g)]
    s[8:11] = torch.tensor([0, -2, n_items + 1])
    w = torch.rand(n_items - 1, generator=g, dtype=torch.float64) + 0.1
    log_q = torch.cat([torch.tensor([-float("inf")], dtype=torch.float64), torch.log(w / w.sum())])
    fix = lambda t: torch.where((t >= 1) & (t < n_items), t, torch.zeros_like(t))  # noqa: E731
    Tp = table[fix(pos)]
    want = sampled_ref(P, Tp, pos, table[fix(s)], s, log_q)
    lists = s.view(1, K).expand(G, K)
    ids, index = list_index(lists, n_items)
    corr = lambda t: torch.where((t >= 1) & (t < n_items), -(log_q[fix(t)] + math.log(K)), torch.zeros((), dtype=torch.float64))  # noqa: E731
    got = ref_loss(P, Tp, pos, table[ids], lists, index, rpl, n_items, bias=corr(s).view(1, K).expand(G, K),
                   pos_bias=corr(pos))
    assert abs(got.item() - want.item()) <= 1e-12 * abs(want.item())
