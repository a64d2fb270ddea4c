"""Softmax cross-entropy over per-list negatives (ops.listed_xent, catalogue.NegativeLists) on the
GPU: the op against the fp64 reference of tests/listed_xent_ref.py over its tile, split and group paths, its edge cases,
its identity with ops.sampled_xent when every list is the same, run-to-run bits and memory; CARCA.listed_softmax_loss and
every parameter gradient against torch.autograd over the oracle; sampling.HardNegativeMiner and
engine.hard_negative_step against the same steps done by hand."""
import math

import pytest
import torch

from carca_replication_amd import CarcaHipError, engine, ops
from carca_replication_amd.catalogue import NegativeLists
from carca_replication_amd.sampling import HardNegativeMiner
from oracle import carca_oracle as O
from tests.listed_xent_ref import ref_loss
from tests.test_hip_catalogue_xent import MODEL_CASES, N_ATTRS, _setup
from tests.test_hip_sampled_xent import _operands as _sampled_operands

pytestmark = pytest.mark.gpu


def _operands(G, rpl, N, d, n_items, seed):
    """test_hip_sampled_xent's operands with a list per group: P ~ N(0, 1), Tp and S ~ N(0, 1) / sqrt(d); about 20 % of
    the rows invalid; a third of each list's entries positives of its own group's rows (accidental hits, some invalid),
    about 10 % no class, duplicates inside and across lists."""
    g = torch.Generator().manual_seed(seed)
    R = G * rpl
    P = torch.randn(R, d, generator=g, dtype=torch.float64)
    Tp = torch.randn(R, d, generator=g, dtype=torch.float64) / d ** 0.5
    pos = torch.randint(1, n_items, (R,), generator=g)
    bad = torch.rand(R, generator=g) < 0.2
    pos[bad] = torch.tensor([0, -3, n_items, n_items + 7])[torch.randint(0, 4, (int(bad.sum()),), generator=g)]
    lists = torch.randint(1, n_items, (G, N), generator=g)
    if N > 2:
        own = torch.randint(0, rpl, (G, N // 3), generator=g) + rpl * torch.arange(G).view(G, 1)
        lists[:, : N // 3] = pos[own]
        lists[:, N - 1] = 0
    bad_e = torch.rand(G, N, generator=g) < 0.1
    lists[bad_e] = torch.tensor([0, -1, n_items, n_items + 3])[torch.randint(0, 4, (int(bad_e.sum()),), generator=g)]
    nl = NegativeLists(lists.cuda(), n_items)
    S = torch.randn(len(nl), d, generator=g, dtype=torch.float64) / d ** 0.5
    bias = torch.randn(G, N, generator=g, dtype=torch.float64) * 0.5
    pos_bias = torch.randn(R, generator=g, dtype=torch.float64) * 0.5
    return P, Tp, S, pos, nl, bias, pos_bias


def _check_op(G, rpl, N, d, n_items=5000, seed=0, with_bias=True):
    P64, T64, S64, pos, nl, bias, pos_bias = _operands(G, rpl, N, d, n_items, seed)
    if not with_bias:
        bias = pos_bias = None
    Pr, Tr, Sr = (x.cuda().requires_grad_(True) for x in (P64, T64, S64))
    want = ref_loss(Pr, Tr, pos, Sr, nl.lists, nl.index, rpl, n_items, bias, pos_bias)
    want.backward()
    P, Tp, S = (x.float().cuda().requires_grad_(True) for x in (P64, T64, S64))
    f = lambda t: None if t is None else t.float().cuda()  # noqa: E731
    got = ops.listed_xent(P, Tp, pos.cuda(), S, nl.lists, nl.index, rpl, f(bias), f(pos_bias), n_items=n_items,
                          csr=(nl.csr_off, nl.csr_ent))
    got.backward()
    w = want.item()
    print(f"listed_xent ({G}, {rpl}, {N}, {d}) n_items {n_items}: loss {got.item():.8g} want {w:.8g}")
    assert abs(got.item() - w) <= 1e-5 * max(abs(w), 0.1), (got.item(), w)
    for name, g, r in (("P", P.grad, Pr.grad), ("Tp", Tp.grad, Tr.grad), ("S", S.grad, Sr.grad)):
        assert g.shape == r.shape, name
        err = float((g.double() - r).abs().max()) if r.numel() else 0.0
        top = float(r.abs().max()) if r.numel() else 0.0
        print(f"  d{name}: err {err:.3g} of max {top:.3g}")
        assert err <= 1e-4 * top + 1e-9, (name, err, top)
    return got


# (G, rows_per_list, N, d): one entry; an odd list and d; a group short of a block; the training shape; a full 64-row
# block and a list of three tiles; a group past one 64-row block; more groups than CUs; a split list with several row
# blocks; many groups with odd sizes
OP_CASES = [(1, 1, 1, 64), (3, 1, 65, 90), (5, 7, 63, 90), (4, 50, 64, 128), (2, 64, 130, 192), (3, 65, 1000, 256),
            (300, 3, 17, 64), (2, 200, 4096, 128), (130, 50, 101, 90)]


@pytest.mark.parametrize("G,rpl,N,d", OP_CASES)
def test_op_matches_fp64_reference(G, rpl, N, d):
    _check_op(G, rpl, N, d, seed=G + rpl + N + d)


def test_op_without_bias_matches_fp64_reference():
    _check_op(5, 7, 63, 90, seed=3, with_bias=False)


def test_op_builds_the_csr_itself_when_not_given():
    P64, T64, S64, pos, nl, _, _ = _operands(5, 7, 63, 90, 5000, 4)
    grads = []
    for csr in (None, (nl.csr_off, nl.csr_ent)):
        P, Tp, S = (x.float().cuda().requires_grad_(True) for x in (P64, T64, S64))
        ops.listed_xent(P, Tp, pos.cuda(), S, nl.lists, nl.index, 7, n_items=5000, csr=csr).backward()
        grads.append(S.grad)
    assert torch.equal(*grads)


def test_op_small_catalogue_most_entries_hits_or_no_class():
    """n_items = 3: most entries are the row's own positive or no class at all; rows whose every entry is masked reduce
    to row loss 0 with the positive alone."""
    _check_op(6, 50, 70, 90, n_items=3, seed=11)


def test_op_no_valid_row_gives_zero_loss_and_gradients():
    P = torch.randn(6, 90, device="cuda", requires_grad=True)
    Tp = torch.randn(6, 90, device="cuda", requires_grad=True)
    nl = NegativeLists(torch.randint(1, 40, (2, 33), device="cuda"), 40)
    S = torch.randn(len(nl), 90, device="cuda", requires_grad=True)
    loss = ops.listed_xent(P, Tp, torch.tensor([0, 0, -1, 40, 0, 47], device="cuda"), S, nl.lists, nl.index, 3, n_items=40)
    loss.backward()
    assert loss.item() == 0.0
    for g in (P.grad, Tp.grad, S.grad):
        assert float(g.abs().max()) == 0.0


def test_op_all_padding_lists():
    """U = 0: every valid row's loss is 0 (the positive alone), dP and dTp are 0 and dS is empty."""
    P = torch.randn(8, 90, device="cuda", requires_grad=True)
    Tp = torch.randn(8, 90, device="cuda", requires_grad=True)
    nl = NegativeLists(torch.tensor([[0, -1, 40, 41, 0]] * 4, device="cuda"), 40)
    assert len(nl) == 0
    S = torch.zeros(0, 90, device="cuda", requires_grad=True)
    pos = torch.tensor([1, 2, 0, 39, 5, 6, 40, 8], device="cuda")
    loss = ops.listed_xent(P, Tp, pos, S, nl.lists, nl.index, 2, pos_bias=torch.randn(8, device="cuda"), n_items=40)
    loss.backward()
    assert loss.item() == 0.0
    assert float(P.grad.abs().max()) == 0.0 and float(Tp.grad.abs().max()) == 0.0
    assert S.grad is None or S.grad.numel() == 0


def test_op_one_shared_list_equals_sampled_xent():
    """Every list the same s_ids, bias and pos_bias the logQ corrections: ops.sampled_xent, an independent kernel -- the
    loss, dP, dTp, and dS once both are scattered to the rows of one item table."""
    G, rpl, K, d, n_items = 68, 50, 1000, 90, 5000
    R = G * rpl
    P64, T64, _, pos, s, log_q = _sampled_operands(R, K, d, n_items, seed=21)
    table = torch.randn(n_items, d, generator=torch.Generator().manual_seed(22), dtype=torch.float64) / d ** 0.5
    s_fix = torch.where((s >= 1) & (s < n_items), s, torch.zeros_like(s))
    P1, Tp1 = (x.float().cuda().requires_grad_(True) for x in (P64, T64))
    S1 = table[s_fix].float().cuda().requires_grad_(True)
    want = ops.sampled_xent(P1, Tp1, pos.cuda(), S1, s.cuda(), log_q.cuda())
    want.backward()
    _, _, bp, bs = ops.sampled_xent_corrections(pos.cuda(), s.cuda(), log_q.cuda())
    nl = NegativeLists(s.cuda().view(1, K).expand(G, K), n_items, bias=bs.view(1, K).expand(G, K))
    P2, Tp2 = (x.float().cuda().requires_grad_(True) for x in (P64, T64))
    S2 = table[nl.ids.cpu().long()].float().cuda().requires_grad_(True)
    got = ops.listed_xent(P2, Tp2, pos.cuda(), S2, nl.lists, nl.index, rpl, nl.bias, bp, n_items=n_items,
                          csr=(nl.csr_off, nl.csr_ent))
    got.backward()
    assert abs(got.item() - want.item()) <= 1e-5 * max(abs(want.item()), 0.1), (got.item(), want.item())
    live = ((s >= 1) & (s < n_items)).cuda()
    dT1 = torch.zeros(n_items, d, dtype=torch.float64, device="cuda").index_add_(0, s_fix.cuda()[live], S1.grad.double()[live])
    dT2 = torch.zeros(n_items, d, dtype=torch.float64, device="cuda").index_add_(0, nl.ids.long(), S2.grad.double())
    for name, a, b in (("P", P2.grad, P1.grad), ("Tp", Tp2.grad, Tp1.grad), ("S", dT2, dT1)):
        err = float((a - b).abs().max())
        assert err <= 1e-4 * float(b.abs().max()) + 1e-9, (name, err, float(b.abs().max()))


def test_op_two_calls_are_bit_identical():
    P64, T64, S64, pos, nl, bias, pos_bias = _operands(68, 50, 4096, 90, 5000, seed=5)
    outs = []
    for _ in range(2):
        P, Tp, S = (x.float().cuda().requires_grad_(True) for x in (P64, T64, S64))
        loss = ops.listed_xent(P, Tp, pos.cuda(), S, nl.lists, nl.index, 50, bias.float().cuda(), pos_bias.float().cuda(),
                               n_items=5000, csr=(nl.csr_off, nl.csr_ent))
        loss.backward()
        outs.append((loss.detach().clone(), P.grad.clone(), Tp.grad.clone(), S.grad.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_op_needs_no_logit_buffer_and_no_gathered_copy():
    """G = 128, rows_per_list = 50, N = 4096, d = 128: the forward and backward calls' memory beyond their inputs (the
    built lists included) and the gradients they return stays within the planned backward scratch plus 1 MB -- whose
    bound, (G N + (splits + 1) R) ld + O(R) words, leaves room for neither an [R, N] logit buffer nor a second [G, N, d]
    copy of the gathered rows."""
    G, rpl, N, d, n_items = 128, 50, 4096, 128, 1_000_001
    R = G * rpl
    g = torch.Generator(device="cuda").manual_seed(0)
    P = torch.randn(R, d, device="cuda", generator=g)
    Tp = torch.randn(R, d, device="cuda", generator=g) / d ** 0.5
    pos = torch.randint(0, n_items, (R,), device="cuda", generator=g).to(torch.int32)
    nl = NegativeLists(torch.randint(1, n_items, (G, N), device="cuda", generator=g), n_items)
    S = torch.randn(len(nl), d, device="cuda", generator=g) / d ** 0.5
    one = torch.ones(1, device="cuda")
    plan = ops.listed_xent_plan(G, rpl, N, len(nl), d, ops.num_cus())
    assert plan["scratch_bwd"] <= (G * N + (plan["splits"] + 1) * R) * d + 4 * R + 1024
    # The caching allocator hands out a cached block whole when what is left of it is under 1 MB, and counts the whole
    # block as allocated.  So the blocks that building the inputs left in the cache are released first (none of them
    # can be handed to the op oversized), and what the returned tensors occupy is read from the allocator after the
    # calls, block slack included, not worked out from their element counts.
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    loss, lse, row_loss = ops.listed_xent_fwd(P, Tp, pos, S, nl.lists, nl.index, rpl, None, None, n_items, d)
    dP, dTp, dS = ops.listed_xent_bwd(P, Tp, pos, S, nl.lists, nl.index, rpl, None, None, n_items,
                                      (nl.csr_off, nl.csr_ent), lse, row_loss, one, d)
    torch.cuda.synchronize()
    peak, held = torch.cuda.max_memory_allocated() - base, torch.cuda.memory_allocated() - base
    # held: the three gradients and the forward's loss, lse and row_loss; only the gradients are taken off
    extra = peak - held + (loss.numel() + lse.numel() + row_loss.numel()) * 4
    print(f"listed_xent memory: peak {peak / 2 ** 20:.2f} MB, held after the calls {held / 2 ** 20:.2f} MB, gradients "
          f"{(dP.numel() + dTp.numel() + dS.numel()) * 4 / 2 ** 20:.2f} MB, extra {extra / 2 ** 20:.2f} MB, planned scratch "
          f"{plan['scratch_bwd'] * 4 / 2 ** 20:.2f} MB")
    assert extra <= 4 * plan["scratch_bwd"] + (1 << 20), (extra / 2 ** 20, plan["scratch_bwd"] * 4 / 2 ** 20)
    assert math.isfinite(loss.item()) and loss.item() > 0


# ---- model level ---------------------------------------------------------------------------------------------------
N_ITEMS, N_LIST = 300, 70


def _draw_lists(pos, n_items=N_ITEMS, N=N_LIST, seed=0, with_bias=True):
    """A list per user with duplicates, hits of the user's own positives and invalid ids; a bias for every entry."""
    g = torch.Generator().manual_seed(seed + 100)
    B, L = pos.shape
    lists = torch.randint(1, n_items, (B, N), generator=g)
    lists[:, :10] = torch.gather(pos, 1, torch.randint(0, L, (B, 10), generator=g))
    lists[:, 10:13] = torch.tensor([0, -2, n_items + 1])
    lists[:, 13] = lists[:, 14]
    bias = torch.randn(B, N, generator=g) * 0.5 if with_bias else None
    return NegativeLists(lists.cuda(), n_items, bias=None if bias is None else bias.cuda())


def _oracle_loss(Pg, cfg, attrs, batch, n_items, nl, masks=None):
    p_x, p_c, pos = batch
    B, L = p_x.shape
    trace = {}
    O.carca_forward(Pg, cfg, (p_x, attrs[p_x], p_c), [(pos, attrs[pos], p_c)], training=True, trace=trace, masks=masks)
    p = trace["p_final"]
    if cfg.decoder == "wdot":  # p[t] * sum_{j<=t} gamma^j, the reference's float32 slot weights (carca.py:376,385-386)
        w = torch.tril((cfg.gamma ** torch.arange(0, L)).unsqueeze(0).expand(L, L)).to(p.dtype).sum(1)
        p = p * w.view(1, L, 1)
    fix = lambda t: torch.where((t >= 1) & (t < n_items), t, torch.zeros_like(t))  # noqa: E731
    ids = nl.ids.cpu().long().view(1, -1)
    S = O.embedding(Pg, cfg, ids, attrs[ids], torch.zeros(1, ids.shape[1], p_c.shape[-1], dtype=torch.float64),
                    O.get_mask(ids, torch.float64), target=True)[0]
    tp = fix(pos)
    Tp = O.embedding(Pg, cfg, tp, attrs[tp], torch.zeros(B, L, p_c.shape[-1], dtype=torch.float64),
                     O.get_mask(tp, torch.float64), target=True)
    bias = None if nl.bias is None else nl.bias.cpu().double()
    return ref_loss(p.reshape(B * L, -1), Tp.reshape(B * L, -1), pos.reshape(-1), S, nl.lists.cpu(), nl.index.cpu(), L,
                    n_items, bias)


def _profile(model, batch):
    p_x, p_c, _ = batch
    a = None if hasattr(model.embeds, "register_attr_table") else torch.zeros(*p_x.shape, N_ATTRS, device="cuda")
    return (p_x.cuda(), a, p_c.float().cuda())


def _run(model, batch, nl):
    model.zero_grad(set_to_none=True)
    loss = model.listed_softmax_loss(_profile(model, batch), batch[2].cuda(), nl)
    loss.backward()
    return loss


def _compare(model, P, cfg, attrs, batch, masks=None, tol=1e-4, with_bias=True):
    nl = _draw_lists(batch[2], seed=cfg.d, with_bias=with_bias)
    loss = _run(model, batch, nl)
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    want = _oracle_loss(Pg, cfg, attrs, batch, N_ITEMS, nl, masks=masks(model) if masks else None)
    want.backward()
    assert abs(loss.item() - want.item()) <= tol * max(abs(want.item()), 1.0), (loss.item(), want.item())
    refs = {n: Pg[n].grad if Pg[n].grad is not None else torch.zeros_like(Pg[n]) for n, _ in model.named_parameters()}
    # (floor: fp32 round-off of the model's largest gradient, for tensors whose exact gradient is 0 -- the key biases)
    floor = 1e-6 * max(float(r.abs().max()) for r in refs.values())
    for name, prm in model.named_parameters():
        ref = refs[name]
        got = prm.grad.cpu().double() if prm.grad is not None else torch.zeros_like(ref)
        err = float((got - ref).abs().max())
        assert err <= tol * float(ref.abs().max()) + floor, (name, err, float(ref.abs().max()))


@pytest.mark.parametrize("emb,dec,enc,nb,d,H", MODEL_CASES, ids=["-".join(map(str, c)) for c in MODEL_CASES])
def test_model_loss_and_gradients_match_oracle(emb, dec, enc, nb, d, H):
    cfg, P, attrs, batch, model = _setup(emb, dec, enc, nb, d, H, 12)
    _compare(model, P, cfg, attrs, batch, with_bias=nb != 1)


def test_model_composed_route_matches_oracle():
    cfg, P, attrs, batch, model = _setup("all", "wdot", "learnable", 2, 64, 2, 70, B=3)
    assert ops.use_composed(64, [2] * 2, 70)
    _compare(model, P, cfg, attrs, batch)


def test_model_dropout_replays_exported_masks():
    p = 0.3
    cfg, P, attrs, batch, model = _setup("all", "dot", "identity", 2, 90, 3, 12, p=p)
    B, L = batch[0].shape
    model._keep_dropout_masks = True
    torch.manual_seed(7)

    def masks(m):
        raw, sc, d = m._last_dropout_masks, 1.0 / (1.0 - p), cfg.d
        f = lambda t: t.cpu().double() * sc  # noqa: E731
        mk = {"embed": f(raw["embed"]).view(B, L, d)}
        for i, b in enumerate(raw["blocks"]):
            mk[f"attn{i}"] = f(b["m_attn"])
            mk[f"ffn1_{i}"] = f(b["m_ffn1"])[:, :d].reshape(B, L, d)
            mk[f"ffn2_{i}"] = f(b["m_ffn2"])[:, :d].reshape(B, L, d)
        return mk

    _compare(model, P, cfg, attrs, batch, masks=masks, tol=2e-4)


@pytest.mark.parametrize("emb,dec", [("all", "dot"), ("attr", "wdot"), ("mlpid", "dot")])
def test_model_full_lists_equal_catalogue_softmax_loss(emb, dec):
    """Every list arange(1, n_items): the loss and every parameter gradient of catalogue_softmax_loss."""
    cfg, P, attrs, batch, model = _setup(emb, dec, "learnable", 2, 64, 2, 12)
    prof, pos = _profile(model, batch), batch[2].cuda()
    model.zero_grad(set_to_none=True)
    full = model.catalogue_softmax_loss(prof, pos)
    full.backward()
    want = {n: q.grad.clone() for n, q in model.named_parameters()}
    model.zero_grad(set_to_none=True)
    lists = torch.arange(1, N_ITEMS, device="cuda").view(1, -1).expand(pos.shape[0], N_ITEMS - 1)
    got = model.listed_softmax_loss(prof, pos, lists)  # (a raw tensor: the lists are built for the call)
    got.backward()
    assert abs(got.item() - full.item()) <= 1e-5 * abs(full.item()), (got.item(), full.item())
    floor = 1e-6 * max(float(g.abs().max()) for g in want.values())
    for n, q in model.named_parameters():
        err = float((q.grad - want[n]).abs().max())
        assert err <= 1e-4 * float(want[n].abs().max()) + floor, (n, err, float(want[n].abs().max()))


def test_model_all_padding_lists_give_zero():
    cfg, P, attrs, batch, model = _setup("all", "dot", "identity", 1, 64, 2, 12)
    nl = NegativeLists(torch.zeros(batch[0].shape[0], 5, dtype=torch.int64, device="cuda"), N_ITEMS)
    loss = _run(model, batch, nl)
    assert loss.item() == 0.0
    assert all(q.grad is None or float(q.grad.abs().max()) == 0.0 for q in model.parameters())


def test_model_deterministic_mode_gives_identical_gradients():
    cfg, P, attrs, batch, model = _setup("all", "dot", "identity", 2, 90, 3, 12)
    nl = _draw_lists(batch[2])
    ops.set_deterministic(True)
    try:
        runs = []
        for _ in range(2):
            loss = _run(model, batch, nl)
            runs.append([loss.detach().clone()] + [p.grad.clone() for p in model.parameters()])
    finally:
        ops.set_deterministic(False)
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_model_errors():
    cfg, P, attrs, batch, model = _setup("all", "dot", "identity", 1, 64, 2, 12)
    prof, pos = _profile(model, batch), batch[2].cuda()
    nl = _draw_lists(batch[2])
    with pytest.raises(CarcaHipError, match="shape"):
        model.listed_softmax_loss(prof, pos[:, 1:], nl)
    with pytest.raises(CarcaHipError, match="built for n_items"):
        model.listed_softmax_loss(prof, pos, _draw_lists(batch[2], n_items=N_ITEMS + 1))
    with pytest.raises(CarcaHipError, match="one list per user"):
        model.listed_softmax_loss(prof, pos, NegativeLists(nl.lists[1:], N_ITEMS))
    with pytest.raises(CarcaHipError, match="NegativeLists or an integer tensor"):
        model.listed_softmax_loss(prof, pos, [1, 2, 3])
    _, _, _, _, m_ca = _setup("all", "ca", "identity", 1, 64, 2, 12)
    with pytest.raises(CarcaHipError, match="CrossAttentionBlock"):
        m_ca.listed_softmax_loss(prof, pos, nl)


# ---- mining and the training step ------------------------------------------------------------------------------------
def _step_batch(batch):
    """The loader's 5-tuple from _setup's (p_x, p_c, pos): the positive half first, then as many negatives."""
    p_x, p_c, pos = batch
    o_x = torch.cat([pos, torch.ones_like(pos)], 1)
    o_c = torch.cat([p_c, p_c], 1).float()
    return tuple(t.cuda() for t in (p_x, p_c.float(), o_x, o_c, (o_x != 0).float()))


def test_miner_never_returns_the_users_profile_or_positives():
    cfg, P, attrs, batch, model = _setup("all", "dot", "identity", 2, 64, 2, 12)
    p_x, _, pos = batch
    nl = HardNegativeMiner(n_hard=40, skip_top=3).mine(model, _profile(model, batch), pos.cuda())
    assert model.training and (nl.G, nl.N) == (p_x.shape[0], 40)
    lists = nl.lists.cpu().long()
    for b in range(p_x.shape[0]):
        own = set(p_x[b].tolist()) | set(pos[b].tolist())
        got = [x for x in lists[b].tolist() if x != 0]
        assert len(got) == 40 and len(set(got)) == 40 and not own & set(got), b
    model.eval()
    _, top = model.retrieve(_profile(model, batch), None, k=43, exclude=torch.cat([p_x, pos], 1).cuda())
    assert torch.equal(top[:, 3:], lists.cuda())


def test_hard_negative_steps_equal_the_steps_by_hand(monkeypatch):
    """Three engine.hard_negative_steps = mine, listed_softmax_loss, backward, optim.step by hand, bit for bit; with the
    item table a touched-row table (engine.SPARSE_TABLE_BYTES = 0) the step announces p_x, the positives and the lists'
    items, stays sparse, and its trajectory equals the dense one.

    The table has 304 x 64 = 19 x 1024 elements on purpose.  optim.Adam's touched-row route always takes the four-float
    path, its dense route takes the one-float path in a partial last 1024-element chunk, and csrc/optim.hip documents
    that the two contract v's update differently; so the optimizer's "touched-row = dense, bit for bit" holds over
    several steps only for a table of whole chunks (C4's 1,000,001 x 128 table is announced, never dense).  At 300
    items the first run of this test found every row with a gradient marked (0 unmarked of 117), equal gradients and
    equal first moments, and 1-ULP differences (7.5e-9) in v and the parameters of rows 290, 297 and 298 -- the partial
    chunk -- from the second step on."""
    from carca_replication_amd.optim import Adam

    n_items = 304
    models, batch5 = [], None
    for _ in range(3):
        cfg, P, attrs, batch, model = _setup("all", "dot", "identity", 2, 64, 2, 12, n_items=n_items)
        models.append(model)
        batch5 = _step_batch(batch)
    opts = [Adam(m.parameters(), lr=1e-2, weight_decay=0.0) for m in models]
    miner = HardNegativeMiner(n_hard=30, n_uniform=8, skip_top=2)
    p_x, p_c, o_x = batch5[:3]
    pos = o_x[:, : o_x.shape[1] // 2]
    ops.set_deterministic(True)  # (gradients without fp32 atomics: the models' gradients are the same bits)
    try:
        for step in range(3):
            torch.manual_seed(step)
            engine.hard_negative_step(models[0], opts[0], batch5, miner)
            torch.manual_seed(step)
            nl = miner.mine(models[1], (p_x, None, p_c), pos)
            opts[1].zero_grad(set_to_none=True)
            models[1].listed_softmax_loss((p_x, None, p_c), pos, nl).backward()
            opts[1].step()
            torch.manual_seed(step)
            monkeypatch.setattr(engine, "SPARSE_TABLE_BYTES", 0)
            engine.hard_negative_step(models[2], opts[2], batch5, miner)
            monkeypatch.undo()
            for (n, a), b, c in zip(models[0].named_parameters(), models[1].parameters(), models[2].parameters()):
                assert torch.equal(a, b) and torch.equal(a, c), (step, n)
    finally:
        ops.set_deterministic(False)
    E = models[2].embeds.items_embed.weight
    mask = opts[2].state[E]["row_touched"]
    assert 0 < int(mask.sum()) < n_items  # still sparse
    assert bool(mask[torch.cat([p_x.reshape(-1), pos.reshape(-1), nl.ids.long()])].all())
    with pytest.raises(CarcaHipError, match="graphed and sharded"):
        engine.hard_negative_step(models[0], opts[0], batch5, miner, sharded=True)
    with pytest.raises(CarcaHipError, match="graphed and sharded"):
        engine.hard_negative_step(models[0], opts[0], batch5, miner, graphed=True)
