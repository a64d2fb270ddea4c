"""train(..., loss="sampled_softmax") and engine.train_step(..., loss="sampled_softmax"): the sampled softmax with the
logQ correction in the training driver, and the proposal sampler on the device."""
import os
import random

import pytest
import torch

from tests.test_hip_catalogue_xent_train import _loaders, _model

pytestmark = pytest.mark.gpu


def test_train_with_sampled_softmax_loss(tmp_path, monkeypatch):
    from carca_replication_amd.optim import Adam
    from carca_replication_amd.sampling import ItemSampler
    from carca_replication_amd.train import train

    monkeypatch.chdir(tmp_path)
    random.seed(0)
    torch.manual_seed(0)
    train_loader, val_loader, attrs, (n_items, n_ctx, n_attrs) = _loaders(tmp_path)
    model = _model(n_items, n_ctx, n_attrs, p=0.2)
    model.embeds.register_attr_table(torch.as_tensor(attrs, dtype=torch.float32).cuda())
    optim = Adam(model.parameters(), lr=1e-3, weight_decay=0.0, betas=(0.9, 0.98))
    counts = torch.arange(n_items) % 7
    for run, sampler in (("run", None), ("run_pop", ItemSampler(n_items, 16, counts=counts, alpha=0.75))):
        train(model=model, train_loader=train_loader, val_loader=val_loader, test_loader=None, device="cuda",
              optim=optim, epochs=4, early_stop=20, datadir=run, verbose=1, loss="sampled_softmax", sampler=sampler)
        logs = [f for f in os.listdir(run) if f.endswith(".csv")]
        rows = [ln.strip().split(";") for ln in open(os.path.join(run, logs[0]))]
        losses = [float(r[3]) for r in rows if r[2] == "train"]
        assert len(losses) == 4 and losses[-1] < losses[0], (run, losses)
    with pytest.raises(Exception, match="graphed"):
        train(model=model, train_loader=train_loader, val_loader=val_loader, test_loader=None, device="cuda",
              optim=optim, epochs=1, datadir="run2", verbose=0, graphed=True, loss="sampled_softmax")


def test_sampled_step_keeps_a_touched_row_table_sparse_and_exact(tmp_path, monkeypatch):
    """With the item table treated as a touched-row table (engine.SPARSE_TABLE_BYTES = 0), the sampled step announces
    p_x, the positives and the samples to optim.Adam.mark_rows: the table is not marked dense, its touched-row mask holds
    exactly those ids, and the step equals a dense Adam step bit for bit."""
    from carca_replication_amd import CarcaHipError, engine, ops
    from carca_replication_amd.optim import Adam
    from carca_replication_amd.sampling import ItemSampler

    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(engine, "SPARSE_TABLE_BYTES", 0)
    train_loader, _, attrs, (n_items, n_ctx, n_attrs) = _loaders(tmp_path)
    batch = [t[:2].cuda() for t in engine.as_batch7(next(iter(train_loader)))]  # (two users: a few of the 60 items)
    torch.manual_seed(1)
    m1 = _model(n_items, n_ctx, n_attrs)
    m2 = _model(n_items, n_ctx, n_attrs)
    m2.load_state_dict(m1.state_dict())
    for m in (m1, m2):
        m.embeds.register_attr_table(torch.as_tensor(attrs, dtype=torch.float32).cuda())
    o1 = Adam(m1.parameters(), lr=1e-2, weight_decay=0.0)
    o2 = Adam(m2.parameters(), lr=1e-2, weight_decay=0.0)
    p_x, p_a, p_c, o_x = batch[:4]
    pos = o_x[:, : o_x.shape[1] // 2]
    sampler = ItemSampler(n_items, 8)
    ops.set_deterministic(True)  # (gradients without fp32 atomics: the two models' gradients are the same bits)
    try:
        torch.manual_seed(5)
        engine.train_step(m1, o1, batch, loss="sampled_softmax", sampler=sampler)
        torch.manual_seed(5)
        samples = sampler.sample()
        o2.zero_grad(set_to_none=True)
        m2.sampled_softmax_loss((p_x, p_a, p_c), pos, samples, sampler.log_q()).backward()
        o2.step()
    finally:
        ops.set_deterministic(False)
    for (n, a), b in zip(m1.named_parameters(), m2.parameters()):
        assert torch.equal(a, b), n
    E = m1.embeds.items_embed.weight
    mask = o1.state[E]["row_touched"]
    want = torch.zeros(n_items, dtype=torch.uint8, device="cuda")
    want[torch.cat([p_x.reshape(-1), pos.reshape(-1), samples.reshape(-1)]).long()] = 1
    assert torch.equal(mask, want)
    assert int(mask.sum()) < n_items  # still sparse: section 13's step would have marked every row
    with pytest.raises(CarcaHipError, match="sharded"):
        engine.train_step(m1, o1, batch, sharded=True, loss="sampled_softmax")


def test_default_sampler_is_uniform_with_at_most_8192_samples():
    from carca_replication_amd import engine

    model = _model(500, 3, 6)
    s = engine.default_sampler(model, "cuda")
    assert s.n_samples == 499 and s._cdf is None
    big = _model(20000, 3, 6)
    assert engine.default_sampler(big, "cuda").n_samples == 8192


@pytest.mark.parametrize("alpha", [None, 0.0, 0.75, 1.0])  # None: counts=None, the torch.randint path default_sampler takes
def test_sampler_draws_follow_q_and_repeat_under_a_seed(alpha):
    from carca_replication_amd.sampling import ItemSampler

    n_items, K = 60, 200_000
    g = torch.Generator().manual_seed(2)
    counts = torch.randint(0, 40, (n_items,), generator=g)
    if alpha is None:
        s = ItemSampler(n_items, K, device="cuda")
        assert s._cdf is None
    else:
        s = ItemSampler(n_items, K, counts=counts, alpha=alpha, device="cuda")
    torch.manual_seed(9)
    a = s.sample()
    torch.manual_seed(9)
    b = s.sample()
    assert a.is_cuda and torch.equal(a, b)
    assert int(a.min()) >= 1 and int(a.max()) < n_items
    obs = torch.bincount(a.cpu(), minlength=n_items)[1:].double()
    exp = s.log_q()[1:].double().exp().cpu() * K
    chi2 = float(((obs - exp) ** 2 / exp).sum())
    # 58 degrees of freedom: the 0.999 quantile is about 99.6
    assert chi2 < 99.6, chi2
