"""The eval-mode SelfAttentionBlock kernel (csrc/sa_eval.hip) lending idle workgroups: with two workgroups per user and the
pads_uniform promise, the second workgroup of a one-tile user (no tile of its own) takes query tiles 0 / 1 of a four-tile
user, up to two donors per recipient, both in user order.  Which workgroup runs a (tile, head) or (tile, feature tile)
job changes no sum, so every case runs with tuning key 23 at 0 (lending) and 1 (the fixed split) and asks for equal
bits, for ops.sa_eval_lent() -- the number of donors that took tiles -- and for the float64 oracle within the tolerance
the other SelfAttentionBlock eval tests use (tests/test_hip_forward.py: 1e-4 absolute on O(1..10) activations).

All cases: d = 90, H = 3 (the <96, 32, 3> kernel), profiles left-padded, leading pad rows of x zero (what the masked
embedding hands the first block)."""
import pytest
import torch

from oracle import carca_oracle as O

pytestmark = pytest.mark.gpu

ACT_ATOL = 1e-4
D, H = 90, 3


@pytest.fixture(scope="module")
def block():
    from carca_replication_amd import modules as M

    torch.manual_seed(29)
    blk = M.SelfAttentionBlock(D, H, 0.0, True).cuda().eval()
    with torch.no_grad():
        for p_ in blk.parameters():
            if p_.dim() == 1:
                p_.add_(0.1 * torch.randn_like(p_))
    P64 = {"encoder.0." + k: v.detach().cpu().double() for k, v in blk.state_dict().items()}
    return blk, P64


def _ids(lens, L):
    lens = torch.as_tensor(lens)
    return (torch.arange(L)[None, :] >= (L - lens)[:, None]).int() * 3


def _x(ids, seed):
    from carca_replication_amd import ops

    dpi, _, _ = ops.padded_dims(D, H)
    B, L = ids.shape
    x = torch.zeros(B, L, dpi)
    x[..., :D] = torch.randn(B, L, D, generator=torch.Generator().manual_seed(seed))
    lead = torch.cumsum(ids != 0, dim=1) == 0
    return torch.where(lead[..., None], torch.zeros(()), x)


def _want(block, ids, x):
    cfg = O.CarcaConfig(d=D, H=H, n_blocks=1)
    return O.sa_block(block[1], cfg, 0, x[..., :D].double(), (ids != 0).double())


def _run(block, ids, x, key, uniform=True):
    """(y on the host, donors that took tiles) of one eager launch with tuning key 23 = `key`."""
    from carca_replication_amd import _lib, ops

    lib = _lib.load()
    lib.carca_set_tuning(ops.TUNE_SA_LEND, key)
    try:
        with torch.no_grad():
            y = ops.sa_block_fwd(x.cuda(), ids.cuda(), block[0].weights_struct(torch.device("cuda")), D, H, True,
                                 pads_uniform=uniform)
        lent = ops.sa_eval_lent()
    finally:
        lib.carca_set_tuning(ops.TUNE_SA_LEND, 0)
    return y.cpu(), lent


def _check(block, ids, x, lent_want, uniform=True, want=None):
    """Both mappings: the count, equal bits, nothing in the padding columns, the oracle.  Returns y."""
    y0, lent0 = _run(block, ids, x, 0, uniform)
    y1, lent1 = _run(block, ids, x, 1, uniform)
    print(f"lent {lent0} (key 0) / {lent1} (key 1), want {lent_want} / 0")
    assert (lent0, lent1) == (lent_want, 0)
    assert torch.equal(y0, y1)
    assert float(y0[..., D:].abs().max()) == 0.0
    want = _want(block, ids, x) if want is None else want
    err = float((y0[..., :D].double() - want).abs().max())
    print(f"max |y - float64 oracle| = {err:.3e}")
    assert err < ACT_ATOL, err
    return y0


LENS_MIXED = [50, 50, 48, 3, 10, 15, 33, 16]  # recipients 50, 50, 48; donors 3, 10, 15; 16 -> 17 rows, two tiles


def test_all_three_splits_in_one_launch(block):
    """Three recipients, three donors: recipient 0 four-way, recipient 1 three-way, recipient 2 on the fixed split; the
    same count with the donors before the recipients and interleaved with them."""
    L = 50
    ids = _ids(LENS_MIXED, L)
    x = _x(ids, 1)
    want = _want(block, ids, x)
    _check(block, ids, x, 3, want=want)
    for perm in ([3, 4, 5, 7, 6, 0, 1, 2], [3, 0, 6, 4, 1, 7, 5, 2], [2, 5, 1, 4, 0, 3, 7, 6]):
        perm = torch.tensor(perm)
        _check(block, ids[perm], x[perm], 3, want=want[perm])


def test_interior_pads_keep_the_plan_and_stay_exact_zeros(block):
    """Zeros inside the kept range of a recipient and of a donor do not shorten a profile: same counts, same bits across
    the key; a masked key's weight is an exact 0 -- another row in its place changes no other row's bits."""
    L = 50
    ids = _ids(LENS_MIXED, L)
    holes = [(0, 10), (0, 30), (0, 47), (4, 45), (4, 48)]  # user 0: a recipient; user 4 (slots 40..49): a donor
    for u, s in holes:
        ids[u, s] = 0
    x = _x(ids, 2)
    y = _check(block, ids, x, 3)
    x2 = x.clone()
    for u, s in holes:
        x2[u, s, :D] = 7.0 * torch.randn(D, generator=torch.Generator().manual_seed(s))
    y2, lent = _run(block, ids, x2, 0)
    assert lent == 3
    keep = torch.ones(ids.shape, dtype=torch.bool)
    for u, s in holes:
        keep[u, s] = False
    assert torch.equal(y[keep], y2[keep])


def test_more_donors_than_needed_and_none(block):
    L = 50
    ids = _ids([5, 50, 3, 15, 1, 0, 9, 12], L)  # one recipient, seven one-tile users (an all-pad profile among them)
    _check(block, ids, _x(ids, 3), 2)
    ids = _ids([50] * 8, L)  # every profile full: no workgroup idle, the fixed split as it was
    _check(block, ids, _x(ids, 4), 0)


@pytest.mark.parametrize("L,lens", [(20, [20, 3, 1, 19, 15, 16, 0, 8]), (17, [17, 17, 3, 17, 1, 17, 16, 15])])
def test_no_recipients(block, L, lens):
    """At most two tiles (L = 20), and L = 17 with full profiles: nobody to lend to."""
    ids = _ids(lens, L)
    _check(block, ids, _x(ids, L), 0)


def test_no_promise_no_lending(block):
    """carca_sa_block_fwd's own eval path passes pads_uniform = 0: no row is re-based, every user has the same tile
    count, nothing is lent."""
    ids = _ids(LENS_MIXED, 50)
    _check(block, ids, _x(ids, 5), 0, uniform=False)


def test_edge_of_the_grid_rule(block):
    """B = 128 = #CUs / 2: still two workgroups per user; one recipient behind / among 127 one-tile users."""
    assert torch.cuda.get_device_properties(0).multi_processor_count == 256
    L = 50
    lens = [3] * 128
    lens[77] = 50
    ids = _ids(lens, L)
    _check(block, ids, _x(ids, 6), 2)
