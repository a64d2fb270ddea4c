"""Host side of the per-item cache of the evaluation feature product (AllEmbedding.feat_cache, modules.py): what its key
follows, the byte budget, and that the cache stays out of pickles.  No GPU."""
import copy
import pickle

import torch

from carca_replication_amd import _lib
from carca_replication_amd import modules as M


def _emb(n_items=50, g=128, n_ctx=2, n_attrs=2048):
    torch.manual_seed(0)
    return M.AllEmbedding(n_items, 8, g, n_ctx, n_attrs, M.IdentityEncoding())


def test_key_follows_weights_table_width_and_stream():
    emb = _emb()
    W = emb.feats_embed.weight
    table = torch.rand(50, 2048)
    key = lambda t=None, n=2048, s=7: M.feat_cache_key(M._WEIGHT_EPOCH[0], W, t, n, s)  # noqa: E731
    k0 = key()
    assert key() == k0
    with torch.no_grad():
        W.mul_(0.5)  # (in place: the version moves, the pointer stays)
    k1 = key()
    assert k1 != k0
    M.note_training_forward()  # (optimizers that do not bump _version: the epoch does)
    k2 = key()
    assert k2 != k1
    with torch.no_grad():
        emb.feats_embed.bias.add_(1.0)  # (the bias is not part of P)
    assert key() == k2
    assert key(t=table) != k2 and key(t=table) == key(t=table)
    assert key(t=table.clone()) != key(t=table)
    kt = key(t=table)
    table.mul_(2.0)
    assert key(t=table) != kt
    assert key(n=1024) != k2 and key(s=8) != k2


def test_budget_counts_the_attribute_copy_only_for_dense_batches(monkeypatch):
    assert M.feat_cache_bytes(12102, 4096, 450) == 12102 * (4096 + 450) * 4
    assert M.feat_cache_bytes(12102, 0, 450) == 12102 * 450 * 4
    assert M.feat_cache_bytes(1 << 20, 4096, 450) > M.FEAT_CACHE_BUDGET  # (2^20 items, dense: never allocated)
    emb = _emb()
    monkeypatch.setattr(M, "FEAT_CACHE_BUDGET", M.feat_cache_bytes(50, 2048, 128) - 1)
    assert emb.feat_cache(2048, None) is None and "_feat_cache" not in emb.__dict__
    assert emb.feat_cache(64, None) is None  # (a K the dedup route never takes)


def test_pickling_and_copying_drop_the_cache():
    emb = _emb()
    emb.__dict__["_feat_cache"] = dict(stream=0, key=("k",), P=torch.zeros(50, 128), state=torch.ones(50, dtype=torch.int32),
                                       A=None, table=None, dirty=True)
    assert "_feat_cache" not in emb.__getstate__()
    assert "_feat_cache" not in pickle.loads(pickle.dumps(emb)).__dict__
    assert "_feat_cache" not in copy.deepcopy(emb).__dict__


def test_entry_points_are_declared():
    for name in ("carca_feat_cache_arm", "carca_feat_dedup_rows_computed", "carca_get_tuning"):
        assert name in _lib.declared_symbols() and name in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.carca_get_tuning(21) == 0 and lib.carca_get_tuning(999) == -1
    assert lib.carca_feat_cache_arm(None) == 0
    bad = _lib.FeatCache()  # (no state, no P: refused)
    bad.n_rows = 4
    import ctypes as C

    assert lib.carca_feat_cache_arm(C.byref(bad)) != 0
