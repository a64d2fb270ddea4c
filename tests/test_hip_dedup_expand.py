"""The expand launch of the evaluation feature product (csrc/feat_dedup.hip: dedup_expand_kernel, with the compact
[W_c^T ; b_f] block that dedup_insert_kernel writes for it): q_r = P[u(r)] + c_r W_c^T + b_f for every kept row, zeros
for id 0, and the hash table handed back clean.

q against a float64 product over the widths the stream-K kernel accepts (g = 450: rows 8-byte aligned only; g = 640;
odd g and odd d: 4-byte accesses), 0 / 1 / 6 / 8 context columns, row counts that are no multiple of the kernel's
rows per workgroup, four segments, B = 512, padding only, user-strided attrs / ctx views; the table after a launch
(the rows the product multiplies, not only q: a stale slot never shows in q); the same bits eager, on a side stream and
in graph replays.  Every case asserts that the dedup path ran."""
import pytest
import torch

from tests.model_util import build_model
from tests.test_hip_feature_dedup import _close

pytestmark = pytest.mark.gpu

NA, L = 4096, 50


def _model(d=90, H=3, g=450, nc=6, n_items=12102, seed=0):
    torch.manual_seed(seed)
    return build_model(dict(d=d, H=H, n_blocks=2), n_items, g, nc, NA, L).cuda().eval()


def _segments(id_mats, nc, gen, strided=False):
    """(ids, attrs, ctx) per id matrix: one random attribute row per distinct id (id 0: zeros), random context.
    strided: attrs / ctx are [:, :T] views of tensors with three more slots per user (a user stride, no copy)."""
    flat = torch.cat([x.reshape(-1) for x in id_mats])
    uniq, inv = torch.unique(flat, return_inverse=True)
    table = torch.rand(len(uniq), NA, generator=gen, device="cuda")
    table[uniq == 0] = 0.0
    a = table[inv]
    c = torch.rand(flat.numel(), nc, generator=gen, device="cuda")
    segs, off = [], 0
    for x in id_mats:
        n, (B, T) = x.numel(), x.shape
        sa, sc = a[off: off + n].view(B, T, NA), c[off: off + n].view(B, T, nc)
        if strided:
            wa, wc = torch.full((B, T + 3, NA), 7.0, device="cuda"), torch.full((B, T + 3, nc), 7.0, device="cuda")
            wa[:, :T], wc[:, :T] = sa, sc
            sa, sc = wa[:, :T], wc[:, :T]
            assert not sa.is_contiguous()
        else:
            sa, sc = sa.contiguous(), sc.contiguous()
        segs.append((x.int().contiguous(), sa, sc))
        off += n
    return segs


def _ids(B, N, groups, gen, lo=1, hi=12102, pad_only=False):
    shapes = [(B, L)] + [(B, N)] * groups
    if pad_only:
        return [torch.zeros(s, dtype=torch.long, device="cuda") for s in shapes]
    xs = [torch.randint(lo, hi, s, generator=gen, device="cuda") for s in shapes]
    lens = torch.randint(3, L + 1, (B,), generator=gen, device="cuda")  # (left padding, as the data loader makes it)
    xs[0] = xs[0] * (torch.arange(L, device="cuda")[None, :] >= (L - lens)[:, None])
    return xs


def _run(model, segs):
    from carca_replication_amd import ops

    d = model.embeds.d
    ops.gemm_rows_log(True)
    with torch.no_grad():
        y = model(profile=segs[0], targets=list(segs[1:]))
    torch.cuda.synchronize()
    log = ops.gemm_rows_log()
    ops.gemm_rows_log(False)
    assert "+dedup" in log, log
    return y.clone(), model.__dict__["_plan"]["zq"][:, d:].clone(), ops.feat_dedup_rows_multiplied()


def _q_ref(model, segs):
    w = model.embeds.feats_embed.weight.double()
    b = model.embeds.feats_embed.bias.double()
    ids = torch.cat([s[0].reshape(-1) for s in segs])
    a = torch.cat([s[1].reshape(-1, NA) for s in segs]).double()
    q = a @ w[:, :NA].T + b
    nc = segs[0][2].shape[-1]
    if nc:
        q = q + torch.cat([s[2].reshape(-1, nc) for s in segs]).double() @ w[:, NA:].T
    return q * (ids != 0)[:, None].double()


def _distinct(segs):
    ids = torch.cat([s[0].reshape(-1) for s in segs])
    return int(torch.unique(ids[ids != 0]).numel())


# (B = 127: 127 * 151 = 19,177 rows and 127 * 170 = 21,590, no multiples of the 16 rows of an expand workgroup)
@pytest.mark.parametrize("name,d,H,g,nc,B,N,groups,kw", [
    ("g450", 90, 3, 450, 6, 127, 101, 1, {}),
    ("g450_whole_workgroups", 90, 3, 450, 6, 128, 101, 1, {}),
    ("g640", 128, 4, 640, 6, 127, 101, 1, {}),
    ("odd_g", 90, 3, 449, 6, 127, 101, 1, {}),
    ("odd_d", 87, 3, 450, 6, 127, 101, 1, {}),
    ("ctx0", 90, 3, 450, 0, 127, 101, 1, {}),
    ("ctx1", 90, 3, 450, 1, 127, 101, 1, {}),
    ("ctx8", 90, 3, 450, 8, 127, 101, 1, {}),
    ("four_segments", 90, 3, 450, 6, 127, 40, 3, {}),
    ("B512", 90, 3, 450, 6, 512, 101, 1, {}),
    ("padding_only", 90, 3, 450, 6, 128, 101, 1, dict(pad_only=True)),
    ("user_strided_views", 90, 3, 450, 6, 127, 101, 1, dict(strided=True)),
])
def test_q_matches_the_float64_product(name, d, H, g, nc, B, N, groups, kw):
    gen = torch.Generator(device="cuda").manual_seed(11)
    model = _model(d, H, g, nc)
    segs = _segments(_ids(B, N, groups, gen, pad_only=kw.get("pad_only", False)), nc, gen, strided=kw.get("strided", False))
    _, q, rows = _run(model, segs)
    _close(q, _q_ref(model, segs))
    assert rows == _distinct(segs)
    ids = torch.cat([s[0].reshape(-1) for s in segs])
    assert not bool(q[ids == 0].any())  # (zeros, bit for bit +0.0 or -0.0 aside: the rows of id 0)


def test_the_table_is_handed_back_clean():
    """Batch A, batch B with other ids, A again, then A's ids in reverse row order, all on one stream.  A slot that kept
    its entry would leave q as it is (the byte compare refuses a stale representative) but the rows would stop merging:
    the rows the product multiplies must stay the number of distinct ids."""
    gen = torch.Generator(device="cuda").manual_seed(5)
    model = _model()
    xa = _ids(128, 101, 1, gen, 1, 6000)
    xb = _ids(128, 101, 1, gen, 6000, 12102)
    A, Bt = _segments(xa, 6, gen), _segments(xb, 6, gen)
    ya, qa, na = _run(model, A)
    _, qb, nb = _run(model, Bt)
    ya2, qa2, na2 = _run(model, A)
    assert torch.equal(qa2, qa) and torch.equal(ya2, ya)
    assert na == na2 == _distinct(A) and nb == _distinct(Bt)
    _close(qb, _q_ref(model, Bt))
    # the same ids at other rows: every group's lowest row moves
    R = [tuple(t.flip(0).flip(1).contiguous() for t in s) for s in A]
    _, qr, nr = _run(model, R)
    assert nr == _distinct(A)
    _close(qr, _q_ref(model, R))


def test_same_bits_eager_side_stream_and_graph_replays():
    gen = torch.Generator(device="cuda").manual_seed(9)
    model = _model()
    segs = _segments(_ids(127, 101, 1, gen), 6, gen)
    y0, q0, _ = _run(model, segs)
    zq = model.__dict__["_plan"]["zq"]
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ys = model(profile=segs[0], targets=list(segs[1:])).clone()
            qs = zq[:, 90:].clone()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        assert torch.equal(ys, y0) and torch.equal(qs, q0)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            yg = model(profile=segs[0], targets=list(segs[1:]))
        assert model.__dict__["_plan"]["zq"] is zq
        for _ in range(3):
            zq.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(yg, y0) and torch.equal(zq[:, 90:], q0)
        del graph
    y1, q1, _ = _run(model, segs)  # (eager again, after the capture's own table and scratch)
    assert torch.equal(y1, y0) and torch.equal(q1, q0)
