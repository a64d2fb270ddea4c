"""The evaluation feature product over distinct attribute rows (csrc/feat_dedup.hip + gemm_rows_skc_kernel, gemm.hip):
q = [a ; c] W_f^T + b_f of every kept row from one representative product per group of equal attribute rows.

Checked at C2 dimensions (n_attrs 4096, g 450: the stream-K kernel's shapes) against a float64 product, on batches with
heavy and no duplication, one id everywhere, padding only, four segments, ids up to 1 M and B = 512; rows of one id whose
bytes differ; run to run, graph replay against eager, dense batch against the attribute table, dedup on against off
(tuning key 20), and the training forward untouched."""
import pytest
import torch

from tests.model_util import build_model

pytestmark = pytest.mark.gpu

D, H, G, NA, NC, L = 90, 3, 450, 4096, 6, 50
DEDUP_KEY = 20


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


def _model(n_items=12102, seed=0):
    torch.manual_seed(seed)
    return build_model(dict(d=D, H=H, n_blocks=2), n_items, G, NC, NA, L).cuda().eval()


def _rows(ids, gen):
    """Dense attribute rows: one random row per distinct id (id 0: zeros)."""
    uniq, inv = torch.unique(ids, return_inverse=True)
    table = torch.rand(len(uniq), NA, generator=gen, device="cuda")
    table[uniq == 0] = 0.0
    return table[inv]


def _batch(kind, B=128, N=101, groups=1, seed=0):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    def ids(shape):
        if kind == "heavy":
            return torch.randint(1, 40, shape, generator=gen, device="cuda")
        if kind == "none":
            return torch.zeros(shape, dtype=torch.long, device="cuda")  # (filled below: all distinct)
        if kind == "same":
            return torch.full(shape, 7, dtype=torch.long, device="cuda")
        if kind == "pad":
            return torch.zeros(shape, dtype=torch.long, device="cuda")
        if kind == "big":
            return torch.randint(1, 1 << 20, shape, generator=gen, device="cuda")
        return torch.randint(1, 12102, shape, generator=gen, device="cuda")  # "mixed": synthetic-like

    shapes = [(B, L)] + [(B, N)] * groups
    xs = [ids(s) for s in shapes]
    if kind == "none":
        total = sum(s[0] * s[1] for s in shapes)
        perm = torch.randperm(total, generator=gen, device="cuda") + 1
        off = 0
        for i, s in enumerate(shapes):
            xs[i] = perm[off: off + s[0] * s[1]].view(s)
            off += s[0] * s[1]
    if kind not in ("pad", "same"):  # left padding of the profiles, as the data loader makes it
        lens = torch.randint(3, L + 1, (B,), generator=gen, device="cuda")
        xs[0] = xs[0] * (torch.arange(L, device="cuda")[None, :] >= (L - lens)[:, None])
    flat = torch.cat([x.reshape(-1) for x in xs])
    a = _rows(flat, gen)
    c = torch.rand(flat.numel(), NC, generator=gen, device="cuda")
    segs, off = [], 0
    for x in xs:
        n = x.numel()
        segs.append((x.int().contiguous(), a[off: off + n].view(*x.shape, NA).contiguous(),
                     c[off: off + n].view(*x.shape, NC).contiguous()))
        off += n
    return segs


def _run(model, segs):
    from carca_replication_amd import ops

    ops.gemm_rows_log(True)
    with torch.no_grad():
        y = model(profile=segs[0], targets=list(segs[1:]))
    torch.cuda.synchronize()
    log = ops.gemm_rows_log()
    ops.gemm_rows_log(False)
    q = model.__dict__["_plan"]["zq"][:, D:].clone()
    return y.clone(), q, log


def _q_ref(model, segs):
    w = model.embeds.feats_embed.weight.double()
    b = model.embeds.feats_embed.bias.double()
    ids = torch.cat([s[0].reshape(-1) for s in segs])
    a = torch.cat([s[1].reshape(-1, NA) for s in segs]).double()
    c = torch.cat([s[2].reshape(-1, NC) for s in segs]).double()
    q = a @ w[:, :NA].T + c @ w[:, NA:].T + b
    return q * (ids != 0)[:, None].double()


def _close(q, ref, tol=1e-5):
    # (fp32 sums of 4096 products against float64: a few 1e-6 of the largest |q| -- the kernel's K split moves them)
    err = (q.double() - ref).abs()
    ok = torch.isnan(q) == torch.isnan(ref)
    assert bool(ok.all())
    err = torch.where(torch.isnan(ref), torch.zeros_like(err), err)
    scale = float(torch.nan_to_num(ref).abs().max()) + 1.0
    assert float(err.max()) <= tol * scale, float(err.max())


@pytest.mark.parametrize("kind,B,groups", [("heavy", 128, 1), ("none", 128, 1), ("same", 128, 1), ("pad", 128, 1),
                                           ("mixed", 128, 3), ("big", 128, 1), ("mixed", 512, 1)])
def test_q_matches_the_float64_product(kind, B, groups):
    N = 101 if groups == 1 else 40
    # (the item table covers every id: the joint embedding gathers its rows)
    n_items = {"big": 1 << 20, "none": B * (L + N * groups) + 2}.get(kind, 12102)
    model = _model(n_items)
    segs = _batch(kind, B=B, N=N, groups=groups, seed=3)
    _, q, log = _run(model, segs)
    assert "+dedup" in log, log
    _close(q, _q_ref(model, segs))


def test_rows_of_one_id_with_different_bytes_are_not_merged():
    """One id in six target slots of one user (same context): the base row, one element one ulp up, +0.0 -> -0.0, and two
    NaN payloads.  Attribute column k carries a weight of 1e3, so a merged ulp row would give the base row's q bit for
    bit; -0.0 and NaN payloads change no value -- there the rows must still come out right."""
    model = _model()
    segs = _batch("mixed", seed=5)
    k, kz, kn = 11, 12, 13
    with torch.no_grad():
        model.embeds.feats_embed.weight[:, k] = 1e3
    x, a, c = segs[1]
    u, slots = 17, [20, 21, 22, 23, 24]
    x[u, slots] = 9999
    base = torch.rand(NA, device="cuda")
    base[k], base[kz] = 1.0, 0.0
    base[kn] = torch.tensor(0x7FC00001, dtype=torch.int32).view(torch.float32)
    for s in slots:
        a[u, s] = base
    a[u, 21, k] = torch.nextafter(torch.tensor(1.0), torch.tensor(2.0)).item()
    a[u, 22, kz] = -0.0
    a[u, 23, kn] = torch.tensor(0x7FC00002, dtype=torch.int32).view(torch.float32)
    a[u, 20, kn] = 0.5  # (20 and 21: finite rows, the ulp pair)
    a[u, 21, kn] = 0.5
    _, q, log = _run(model, segs)
    assert "+dedup" in log
    r = lambda s: B_L + u * 101 + s  # noqa: E731
    B_L = segs[0][0].numel()
    assert not torch.equal(q[r(20)], q[r(21)])
    ref = _q_ref(model, segs)
    _close(q, ref)
    assert bool(torch.isnan(q[r(22)]).all()) and bool(torch.isnan(q[r(23)]).all())


def test_same_bits_run_to_run_graph_and_table(tuning):
    from carca_replication_amd.synth import eval_batch

    model = _model()
    profile, target, table = eval_batch(128, L, 101, 12102, NA, NC, seed=1234)
    p = tuple(t.cuda() for t in profile)
    t = tuple(t.cuda() for t in target)
    with torch.no_grad():
        y0 = model(profile=p, targets=[t]).clone()
        y1 = model(profile=p, targets=[t]).clone()
        assert torch.equal(y0, y1)
        q0 = model.__dict__["_plan"]["zq"][:, D:].clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            model(profile=p, targets=[t])
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            yg = model(profile=p, targets=[t])
        for _ in range(3):
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(yg, y0)
        del graph
        model.embeds.register_attr_table(table.cuda())
        yt = model(profile=(p[0], None, p[2]), targets=[(t[0], None, t[2])]).clone()
        assert torch.equal(yt, y0)
        model.embeds.register_attr_table(None)
        tuning(DEDUP_KEY, 1)
        yo = model(profile=p, targets=[t]).clone()
        qo = model.__dict__["_plan"]["zq"][:, D:].clone()
    # (the same fp32 sums split at other K steps: the stream-K cuts follow the number of rows multiplied)
    assert float((q0 - qo).abs().max()) <= 1e-5 * (1.0 + float(qo.abs().max()))
    assert float((y0 - yo).abs().max()) <= 1e-5 * (1.0 + float(yo.abs().max()))
    # the positive's rank among its candidates, except where the two scores are within the difference of the builds
    gap = (yo - yo[:, :1]).abs()
    tie = (gap <= 2 * float((y0 - yo).abs().max())).sum(1) > 1
    r0 = (y0 > y0[:, :1]).sum(1)
    ro = (yo > yo[:, :1]).sum(1)
    assert torch.equal(r0[~tie], ro[~tie])


def test_training_forward_takes_no_dedup(tuning):
    """The training forward (saves for the backward) keeps the product over every kept row: the same bits with the switch
    on and off, no dedup launch in the log, and the same gradients (to the order of the backward's fp32 atomics)."""
    from carca_replication_amd import modules as M
    from carca_replication_amd import ops
    from carca_replication_amd.synth import eval_batch

    profile, target, _ = eval_batch(128, L, L, 12102, NA, NC, seed=7)
    p = tuple(t.cuda() for t in profile)
    t = tuple(t.cuda() for t in target)
    y_true = (p[0] != 0).int()
    out = []
    for off in (0, 1):
        tuning(DEDUP_KEY, off)
        model = _model().train()
        ops.gemm_rows_log(True)
        y = model(profile=p, targets=[t])
        M.BinaryCrossEntropy()(y, y_true, M.get_mask(t[0])).backward()
        torch.cuda.synchronize()
        log = ops.gemm_rows_log()
        ops.gemm_rows_log(False)
        assert "+dedup" not in log
        out.append((y.detach().clone(), {n: q.grad.clone() for n, q in model.named_parameters()}))
    assert torch.equal(out[0][0], out[1][0])
    for n in out[0][1]:
        a, b = out[0][1][n], out[1][1][n]
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()) + 1e-9, n
