"""train(..., loss="softmax") and engine.train_step(..., loss="softmax"): the full-catalogue softmax objective in the
training driver."""
import os
import random

import pytest
import torch

from tests.test_train_driver import _write_dataset

pytestmark = pytest.mark.gpu


def _model(n_items, n_ctx, n_attrs, d=64, H=2, p=0.0):
    import torch.nn as nn

    from carca_replication_amd.modules import CARCA, AllEmbedding, DotProduct, IdentityEncoding, SelfAttentionBlock

    emb = AllEmbedding(n_items, d, 48, n_ctx, n_attrs, IdentityEncoding())
    enc = nn.ModuleList([SelfAttentionBlock(d, H, p, True) for _ in range(2)])
    return CARCA(d=d, p=p, emb=emb, enc=enc, dec=DotProduct()).to("cuda")


def _loaders(tmp_path):
    from torch.utils.data import DataLoader

    from src.data import CARCADataset, load_attrs, load_ctx, load_profiles, set_datapath

    _write_dataset(str(tmp_path))
    set_datapath(str(tmp_path))
    attrs, ctx = load_attrs("attrs.dat"), load_ctx("ctx.dat")
    user_ids, item_ids, profiles = load_profiles("profiles.txt")
    mk = lambda mode: CARCADataset(user_ids=user_ids, item_ids=item_ids, profiles=profiles, attrs=attrs, ctx=ctx,  # noqa: E731
                                   profile_seq_len=8, target_seq_len=20, mode=mode, test=True)
    dims = (attrs.shape[0], next(iter(ctx.values())).shape[0], attrs.shape[1])
    return (DataLoader(mk("train"), batch_size=16, shuffle=True, num_workers=0),
            DataLoader(mk("val"), batch_size=16, shuffle=False, num_workers=0), attrs, dims)


def test_train_with_softmax_loss(tmp_path, monkeypatch):
    from carca_replication_amd.optim import Adam
    from carca_replication_amd.train import train

    monkeypatch.chdir(tmp_path)
    random.seed(0)
    torch.manual_seed(0)
    train_loader, val_loader, attrs, (n_items, n_ctx, n_attrs) = _loaders(tmp_path)
    model = _model(n_items, n_ctx, n_attrs, p=0.2)
    model.embeds.register_attr_table(torch.as_tensor(attrs, dtype=torch.float32).cuda())
    optim = Adam(model.parameters(), lr=1e-3, weight_decay=0.0, betas=(0.9, 0.98))
    train(model=model, train_loader=train_loader, val_loader=val_loader, test_loader=None, device="cuda", optim=optim,
          epochs=4, early_stop=20, datadir="run", verbose=1, loss="softmax")
    logs = [f for f in os.listdir("run") if f.endswith(".csv")]
    rows = [ln.strip().split(";") for ln in open(os.path.join("run", logs[0]))]
    losses = [float(r[3]) for r in rows if r[2] == "train"]
    assert len(losses) == 4 and losses[-1] < losses[0], losses
    assert any(f.endswith(".pth") for f in os.listdir("run"))
    with pytest.raises(Exception, match="graphed"):
        train(model=model, train_loader=train_loader, val_loader=val_loader, test_loader=None, device="cuda",
              optim=optim, epochs=1, datadir="run2", verbose=0, graphed=True, loss="softmax")


def test_softmax_step_updates_a_touched_row_table_densely(tmp_path, monkeypatch):
    """With the item table treated as a touched-row table (engine.SPARSE_TABLE_BYTES = 0: BCE steps announce their rows to
    optim.Adam.mark_rows), the softmax step announces none, and so equals a dense Adam step bit for bit."""
    from carca_replication_amd import CarcaHipError, engine, ops
    from carca_replication_amd.optim import Adam

    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(engine, "SPARSE_TABLE_BYTES", 0)
    train_loader, _, attrs, (n_items, n_ctx, n_attrs) = _loaders(tmp_path)
    batch = [t.cuda() for t in engine.as_batch7(next(iter(train_loader)))]
    torch.manual_seed(1)
    m1 = _model(n_items, n_ctx, n_attrs)
    m2 = _model(n_items, n_ctx, n_attrs)
    m2.load_state_dict(m1.state_dict())
    for m in (m1, m2):
        m.embeds.register_attr_table(torch.as_tensor(attrs, dtype=torch.float32).cuda())
    o1 = Adam(m1.parameters(), lr=1e-2, weight_decay=0.0)
    o2 = Adam(m2.parameters(), lr=1e-2, weight_decay=0.0)
    p_x, p_a, p_c, o_x = batch[:4]
    ops.set_deterministic(True)  # (gradients without fp32 atomics: the two models' gradients are the same bits)
    try:
        engine.train_step(m1, o1, batch, loss="softmax")
        o2.zero_grad(set_to_none=True)
        m2.catalogue_softmax_loss((p_x, p_a, p_c), o_x[:, : o_x.shape[1] // 2]).backward()
        o2.step()
    finally:
        ops.set_deterministic(False)
    for (n, a), b in zip(m1.named_parameters(), m2.parameters()):
        assert torch.equal(a, b), n
    E0 = m1.embeds.items_embed.weight.detach().clone()
    untouched = torch.ones(n_items, dtype=torch.bool, device="cuda")
    untouched[torch.cat([p_x.reshape(-1), o_x.reshape(-1)]).long()] = False
    untouched[0] = False
    engine.train_step(m1, o1, batch, loss="softmax")  # rows outside the batch move too
    assert bool(untouched.any()) and float((m1.embeds.items_embed.weight - E0)[untouched].abs().max()) > 0
    with pytest.raises(CarcaHipError, match="sharded"):
        engine.train_step(m1, o1, batch, sharded=True, loss="softmax")
    with pytest.raises(ValueError):
        engine.train_step(m1, o1, batch, loss="hinge")
