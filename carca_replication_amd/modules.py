"""Host-side mirror of the reference's model surface (src/carca.py, src/abstract.py, src/utils.py).

Same class names, constructor signatures, attribute names (hence identical ``state_dict`` keys and
shapes), same parameter-creation order (hence identical weights under the
same ``torch.manual_seed``) and the same ``forward`` contracts -- but every forward runs the
hand-written gfx950 kernels behind the C ABI (include/carca_hip.h).  There is NO eager/ATen
implementation of the model math in this file: called with CPU tensors, or without the HIP
library, the modules raise ``CarcaHipError``.

reference                                     here
---------                                     ----
get_mask                utils.py:6-7          folded into every kernel as (ids != 0)
AllEmbedding.forward    carca.py:85-95        ops.embed_fwd        (csrc/embed.hip)
SelfAttentionBlock      carca.py:297-318      ops.sa_block_fwd     (csrc/sa_block.hip)
CARCA.norm + CrossAttentionBlock carca.py:421,338-349  ops.cross_score_fwd (csrc/cross_score.hip)
CARCA.forward           carca.py:411-431      CARCA.forward below: 1 pack + 3 embed + n_blocks + 1 launches
BinaryCrossEntropy      carca.py:441-444      ops.bce_fwd          (csrc/loss_metrics.hip)
AttrCtx/Attr/Id/MLPId embeddings carca.py:98-198   the same row GEMM with terms removed (ops.gemm_rows)
DotProduct / WeightedDotProduct  carca.py:352-399  ops.dot_score_fwd (+ layernorm_fwd, slot_decay_scale, l2norm; csrc/decoders.hip)
"""
from __future__ import annotations

import math
from abc import ABC, abstractmethod
from functools import partial
from typing import Iterable, List, Optional, Tuple

import torch
import torch.nn as nn
from torch import Tensor

from . import _lib, catalogue, ops
from ._lib import CarcaHipError

# ------------------------------------------------------------------------------------------------
# plug-in interfaces (abstract.py:8-50)
# ------------------------------------------------------------------------------------------------


class Model(nn.Module, ABC):
    """abstract.py:8-14"""

    @abstractmethod
    def forward(self, profile: Tuple[Tensor, Tensor, Tensor], targets: List[Tuple[Tensor, Tensor, Tensor]]) -> Tensor:
        ...


class Embedding(nn.Module, ABC):
    """abstract.py:17-23"""

    @abstractmethod
    def forward(self, x: Tensor, a: Tensor, c: Tensor, mask: Tensor, target: bool) -> Tensor:
        ...


class Encoding(nn.Module, ABC):
    """abstract.py:26-32"""

    @abstractmethod
    def forward(self, x: Tensor) -> Tensor:
        ...


class Encoder(nn.Module, ABC):
    """abstract.py:35-41"""

    @abstractmethod
    def forward(self, x: Tensor, mask: Tensor) -> Tensor:
        ...


class Decoder(nn.Module, ABC):
    """abstract.py:44-50"""

    @abstractmethod
    def forward(self, o: Tensor, o_mask: Tensor, p: Tensor, p_mask: Tensor) -> Tensor:
        ...


def get_mask(input: Tensor) -> Tensor:
    """utils.py:6-7.  Kept for callers (train.py:45,92); the kernels derive the mask from the ids."""
    return torch.where(input == 0.0, 0.0, 1.0)


def to(*tensors: Tensor, device: str) -> Tuple[Tensor, ...]:
    """utils.py:10-11 (None entries -- the attribute slots of an ids-only batch -- pass through)"""
    return tuple(t if t is None else t.to(device) for t in tensors)


# ------------------------------------------------------------------------------------------------
# encodings (carca.py:15-60): an additive [T, d] table, folded into the embed kernel's epilogue
# ------------------------------------------------------------------------------------------------


def _no_standalone_grad(x: Tensor, module: nn.Module) -> None:
    if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in module.parameters())):
        raise CarcaHipError(f"{type(module).__name__}.forward on its own is built for inference (torch.no_grad()): the "
                            "backward pass of the hot path runs through CARCA.forward")


class IdentityEncoding(Encoding):
    def position_table(self, T: int) -> Optional[Tensor]:
        return None

    def forward(self, x: Tensor) -> Tensor:
        return x


class LearnableEncoding(Encoding):
    def __init__(self, d: int, max_len: int):
        super().__init__()
        self.max_len = max_len
        self.encoding = nn.Embedding(max_len, d)
        nn.init.xavier_uniform_(self.encoding.weight)

    def position_table(self, T: int) -> Tensor:
        if T > self.max_len:
            raise CarcaHipError(f"sequence length {T} exceeds LearnableEncoding.max_len={self.max_len}")
        return self.encoding.weight[:T]

    def forward(self, x: Tensor) -> Tensor:
        """Stand-alone use of the ABC (abstract.py:31, carca.py:25-31): x [B, T, d] + encoding[:T].  Inside CARCA the
        table rides in the embedding GEMM's epilogue instead.  Differentiable in x and in the table."""
        table = self.position_table(x.shape[1])
        if torch.is_grad_enabled() and (x.requires_grad or table.requires_grad):
            from .autograd import add_positions_with_grad

            return add_positions_with_grad(x, table)
        return ops.add_positions(x, table)


class PositionalEncoding(Encoding):
    def __init__(self, d_model: int, max_len: int):
        super().__init__()
        position = torch.arange(max_len).unsqueeze(1)
        div_term = torch.exp(torch.arange(0, d_model, 2) * (-math.log(10000.0) / d_model))
        pe = torch.zeros(1, max_len, d_model)
        pe[0, :, 0::2] = torch.sin(position * div_term)
        pe[0, :, 1::2] = torch.cos(position * div_term)
        self.register_buffer("pe", pe)

    def position_table(self, T: int) -> Tensor:
        if T > self.pe.shape[1]:
            raise CarcaHipError(f"sequence length {T} exceeds PositionalEncoding.max_len={self.pe.shape[1]}")
        return self.pe[0, :T]

    def forward(self, x: Tensor) -> Tensor:
        """Stand-alone use of the ABC (abstract.py:31, carca.py:54-60): x [B, T, d] + pe[:, :T]."""
        if torch.is_grad_enabled() and x.requires_grad:
            from .autograd import add_positions_with_grad

            return add_positions_with_grad(x, self.position_table(x.shape[1]))
        return ops.add_positions(x, self.position_table(x.shape[1]))


# ------------------------------------------------------------------------------------------------
# AllEmbedding (carca.py:66-95)
# ------------------------------------------------------------------------------------------------


def _position_table(enc: Encoding, T: int) -> Optional[Tensor]:
    if hasattr(enc, "position_table"):
        return enc.position_table(T)
    raise CarcaHipError(f"encoding {type(enc).__name__} has no position_table(); cannot be fused")


def _segs_pos(enc: Encoding, segs) -> Optional[Tensor]:
    """Position table [T, d] for the profile segment(s) of `segs`, or None (targets never get one, carca.py:91)."""
    if any(not tgt for (_, _, _, tgt) in segs):
        T = next(x.shape[1] for (x, _, _, tgt) in segs if not tgt)
        return _position_table(enc, T)
    return None


def _pos_grad(enc: Encoding, de_profile: Tensor, ids: Tensor, d: int, L: int, gbp) -> None:
    """d LearnableEncoding.encoding.weight[t] += sum over users of (d e * mask)[t]  (carca.py:25-31)."""
    if hasattr(enc, "encoding"):
        ops.colsum(de_profile, d, gbp[id(enc.encoding.weight)], ids=ids, T=L)


def _rows(x: Tensor) -> int:
    return x.numel()


# ---- item-side tables of full-catalogue recommendation (CARCA.recommend) ----------------------
# In eval mode every embedding is affine in the context: e(i, c) = T[i] + M c for i != 0 (targets carry no position term,
# carca.py:91).  T = the class's own embed_segments over one target segment ids = arange(n_items) with zero context, M
# composed from its weights with carca_gemm_rows.  Cached per weight version like every other derived copy (the key of
# _PackedModule._packed plus the identity of the registered attribute table); kept out of pickles.
_TABLE_KEYS = ("_item_table_cache", "_ctx_matrix_cache", "_reco_cache", "_item_rnorm_cache")


def _cached_table(module: nn.Module, slot: str, params, extra: tuple, build, keep=None):
    """keep: an object whose id() is part of `extra` (the attribute table): referenced by the cache, so that the id
    cannot be reused by another tensor while the entry lives."""
    key = (_WEIGHT_EPOCH[0],) + tuple((p.data_ptr(), p._version) for p in params) + extra
    cache = module.__dict__.get(slot)
    if cache is not None and cache[0] == key:
        return cache[1]
    value = build()
    module.__dict__[slot] = (key, value, keep)
    return value


def _item_rnorm(module: nn.Module, T: Tensor) -> Tensor:
    """r [n_items] = 1 / max(||T[i]||, 1e-12) for T = module.item_table(): a derived copy under the item table's own key
    (the entry references T, so a new table is a new entry)."""
    tc = module.__dict__.get("_item_table_cache")
    key = tc[0] if tc is not None and tc[1] is T else None
    cache = module.__dict__.get("_item_rnorm_cache")
    if cache is not None and key is not None and cache[0] == key and cache[2] is T:
        return cache[1]
    r = catalogue.row_rnorm(T, module.d)
    module.__dict__["_item_rnorm_cache"] = (key, r, T)
    return r


def _need_attr_table(module: nn.Module, what: str) -> Tensor:
    table = module.attr_table()
    if table is None:
        raise CarcaHipError(f"{type(module).__name__}.{what}: no attribute table registered -- call "
                            "register_attr_table(attrs) with the [n_items, n_attrs] item-attribute matrix first")
    return table


def _target_table(module: nn.Module, n_items: int, a: Optional[Tensor], n_ctx: int, dev) -> Tensor:
    """T [n_items, row_ld(d)]: embed_segments over ids = arange(n_items) as one target segment, zero context."""
    x = torch.arange(n_items, dtype=torch.int32, device=dev).view(1, n_items)
    c = torch.zeros(1, n_items, n_ctx, dtype=torch.float32, device=dev)
    ld = ops.row_ld(module.d)
    es, _ = module.embed_segments([(x, a, c, True)], ld_e=ld)
    return es[0].reshape(n_items, ld)


def _drop_tables(state: dict) -> dict:
    for k in _TABLE_KEYS:
        state.pop(k, None)
    return state


# the per-item cache of the evaluation feature product (AllEmbedding.feat_cache): what its tensors may take, in bytes
FEAT_CACHE_BUDGET = 2 << 30


def feat_cache_bytes(n_items: int, n_attrs_dense: int, g: int) -> int:
    """P_c [n_items, g] + A_c [n_items, n_attrs] (dense batches; 0 columns on the table path), fp32."""
    return n_items * (n_attrs_dense + g) * 4


def feat_cache_key(epoch: int, W: Tensor, table: Optional[Tensor], n_attrs: int, stream: int) -> tuple:
    """What a filled entry depends on besides its own attribute row: W_a's version (with the epoch every training forward
    advances: not every optimizer bumps _version), which attribute table the rows come from, and the stream the fills
    and the reads are ordered on.  The bias and the context columns are not part of P."""
    return (epoch, W.data_ptr(), W._version, None if table is None else (id(table), table.data_ptr(), table._version),
            int(n_attrs), stream)


class AllEmbedding(Embedding):
    def __init__(self, n_items: int, d: int, g: int, n_ctx: int, n_attrs: int, enc: Encoding):
        super().__init__()
        self.d = d
        self.enc = enc
        self.items_embed = nn.Embedding(num_embeddings=n_items, embedding_dim=d, padding_idx=0)
        self.feats_embed = nn.Linear(in_features=n_ctx + n_attrs, out_features=g)
        self.joint_embed = nn.Linear(in_features=g + d, out_features=d)
        for m in (self.items_embed, self.feats_embed, self.joint_embed):
            nn.init.xavier_uniform_(m.weight)
        with torch.no_grad():
            self.items_embed.weight[0].zero_()
        nn.init.zeros_(self.feats_embed.bias)
        nn.init.zeros_(self.joint_embed.bias)

    def __getstate__(self):  # keep device-side caches (attribute table, folded weights) out of checkpoints
        state = dict(super().__getstate__())
        state.pop("_attr_table", None)
        state.pop("_fold_cache", None)
        state.pop("_split_cache", None)
        state.pop("_wj_t", None)
        state.pop("_fold_train", None)
        state.pop("_wf_t", None)
        state.pop("_ztab_cache", None)
        state.pop("_feat_cache", None)
        return _drop_tables(state)

    def register_attr_table(self, attrs: Optional[Tensor]) -> None:
        """API-compatible extension: keep the item-attribute matrix [n_items, n_attrs] (row 0 = pad,
        exactly `load_attrs`' output, data.py:28-35) on the device.  Afterwards `a` may be None in forward():
        the rows are gathered by item id inside the feature GEMM, so no dense [B, T, n_attrs] batch tensor is
        built, shipped over PCIe or read from HBM.  Valid because the dataset always sets a = attrs[x]
        (data.py:119-132,167-187).  Pass None to unregister."""
        if attrs is None:
            self.__dict__.pop("_attr_table", None)
            return
        if attrs.dim() != 2 or attrs.shape[1] > self.feats_embed.in_features:
            raise CarcaHipError("register_attr_table: expected [n_items, n_attrs] with n_attrs <= feats_embed.in_features")
        self.__dict__["_attr_table"] = attrs.detach().to(self.items_embed.weight.device, torch.float32).contiguous()

    def attr_table(self) -> Optional[Tensor]:
        return self.__dict__.get("_attr_table")

    def folded_weights(self):
        """(W_c [d, ldw], bias_c [d]) with W_c = W_jq W_f and bias_c = W_jq b_f + b_j, composed on the device with
        carca_gemm_rows and cached per weight version (inference only: see CarcaForwardDesc.fold_wc)."""
        prm = (self.feats_embed.weight, self.feats_embed.bias, self.joint_embed.weight, self.joint_embed.bias)
        key = (_WEIGHT_EPOCH[0],) + tuple((p.data_ptr(), p._version) for p in prm)
        cache = self.__dict__.get("_fold_cache")
        if cache is not None and cache[0] == key:
            return cache[1], cache[2]
        Wf, bf, Wj, bj = (p.detach() for p in prm)
        d, g, F = self.d, Wf.shape[0], Wf.shape[1]
        wf_t = ops.PackedWeights([ops.PackItem(Wf, F, g, transposed=True)], Wf.device)  # Bt[n = F][k = g]
        wf_t.pack()
        wjq = Wj[:, d:]  # [d, g] view, row stride d + g
        ldw = ((F + 3) // 4) * 4
        (wc,) = ops.gemm_rows([dict(a0=wjq)], wf_t.view(0), F, g, ldw)
        (bc,) = ops.gemm_rows([dict(a0=wjq, add=bj.view(d, 1))], bf.view(1, g), 1, g, 4)
        bias_c = bc[:, 0].contiguous()
        self.__dict__["_fold_cache"] = (key, wc, bias_c)
        self.__dict__["_wf_t"] = wf_t  # [F, g] transposed copy, reused by the re-associated backward of the same step
        return wc, bias_c

    def z_table(self) -> Tensor:
        """sqrt(d) E W_jz^T, [n_items, d]: the item term of joint_embed (carca.py:87-89) per ITEM instead of per batch row,
        composed on the device with carca_gemm_rows and cached per weight version (inference only: CarcaForwardDesc.z_table
        -- the joint product then runs over q's columns and adds row `id` of this table; no gather launch, no z columns)."""
        prm = (self.items_embed.weight, self.joint_embed.weight)
        key = (_WEIGHT_EPOCH[0],) + tuple((p.data_ptr(), p._version) for p in prm)
        cache = self.__dict__.get("_ztab_cache")
        if cache is not None and cache[0] == key:
            return cache[1]
        E, Wj = (p.detach() for p in prm)
        d = self.d
        (zt,) = ops.gemm_rows([dict(a0=E)], Wj[:, :d], d, d, d, alpha=float(d) ** 0.5)
        self.__dict__["_ztab_cache"] = (key, zt)
        return zt

    def feat_cache(self, n_attrs: int, table: Optional[Tensor]):
        """The per-item cache of the evaluation feature product's attribute part, P[i] = attrs[i] W_a^T, as the
        _lib.FeatCache the next carca_forward is armed with, or None where the forward runs without one.

        Three tensors owned by this module, allocated on the first eligible call and kept out of pickles: P_c
        [n_items, g], state [n_items] (0 empty, 1 filled) and, for dense batches (table None), A_c [n_items, n_attrs], the
        attribute row each entry was computed from -- the kernels compare a batch row's bytes with it before they use
        an entry.  The kernels fill entries; this function empties them all (one memset of state) whenever the key
        changes: (_WEIGHT_EPOCH, data_ptr, _version) of feats_embed.weight, the identity and version of the attribute
        table, n_attrs, the stream.  None: under stream capture, on any stream but the one the cache was created on, with
        tuning key 21 = 1, and where the tensors would exceed FEAT_CACHE_BUDGET bytes."""
        W = self.feats_embed.weight
        g, n_items = W.shape[0], self.items_embed.num_embeddings
        dense = table is None
        # (where the product can run over distinct rows at all: gemm_rows_skc_kernel's K and N, csrc/gemm.hip)
        if n_attrs < 2048 or g <= 96 or ops.get_tuning(ops.TUNE_FEAT_CACHE) == 1:
            return None
        if feat_cache_bytes(n_items, n_attrs if dense else 0, g) > FEAT_CACHE_BUDGET:
            return None
        if torch.cuda.is_current_stream_capturing():
            return None
        stream = ops._stream()
        c = self.__dict__.get("_feat_cache")
        if c is not None and (c["P"].device != W.device or c["P"].shape != (n_items, g)):
            c = None  # (the module moved or changed shape: a new cache)
        if c is not None and c["stream"] != stream:
            return None
        if c is None:
            c = dict(stream=stream, key=None, A=None, table=None, dirty=False,
                     P=torch.empty(n_items, g, dtype=torch.float32, device=W.device),
                     state=torch.zeros(n_items, dtype=torch.int32, device=W.device))
            self.__dict__["_feat_cache"] = c
        if dense and (c["A"] is None or c["A"].shape[1] != n_attrs):
            c["A"] = torch.empty(n_items, n_attrs, dtype=torch.float32, device=W.device)
        key = feat_cache_key(_WEIGHT_EPOCH[0], W, table, n_attrs, stream)
        if c["key"] != key:
            if c["dirty"]:  # (entries filled under another key: all empty again, the data stays)
                c["state"].zero_()
            c["key"], c["table"], c["dirty"] = key, table, True  # (the table is referenced: its id cannot be reused)
        fc = _lib.FeatCache()
        fc.p_c, fc.state, fc.n_rows, fc.ld_p = c["P"].data_ptr(), c["state"].data_ptr(), n_items, g
        fc.a_c, fc.ld_a = (c["A"].data_ptr(), n_attrs) if dense else (None, 0)
        fc.table = None if dense else table.data_ptr()
        return fc

    def _pos(self, T: int) -> Optional[Tensor]:
        return _position_table(self.enc, T)

    def item_table(self) -> Tensor:
        """T [n_items, row_ld(d)] = e(i, c = 0) for every item (row 0 = 0): the forward's own embedding of a target row."""
        table = _need_attr_table(self, "item_table")
        prm = cached_parameters(self)
        n_ctx = self.feats_embed.in_features - table.shape[1]
        return _cached_table(self, "_item_table_cache", prm, (id(table),), lambda: _target_table(
            self, self.items_embed.num_embeddings, None, n_ctx, self.items_embed.weight.device), keep=table)

    def context_matrix(self, n_ctx: int) -> Optional[Tensor]:
        """M [d, n_ctx] = W_jq W_f[:, n_attrs:] (e(i, c) = T[i] + M c), or None without context."""
        if n_ctx == 0:
            return None
        F = self.feats_embed.in_features
        wc, _ = self.folded_weights()
        return wc[:, F - n_ctx: F]

    def bind_split_weights(self, n_attrs: int) -> None:
        """Opt-in split-precision feature GEMM (ops.set_feature_gemm_precision): hand the library the packed 16-bit planes
        of feats_embed.weight[:, :n_attrs], prepared once per weight version (same key as every other packed copy)."""
        mode = ops.feature_gemm_mode()
        if mode == 0:
            return
        W = self.feats_embed.weight
        key = (_WEIGHT_EPOCH[0], W.data_ptr(), W._version, mode, int(n_attrs))
        cache = self.__dict__.get("_split_cache")
        if cache is None or cache[0] != key:
            cache = (key, ops.split_pack(W, n_attrs, mode))
            self.__dict__["_split_cache"] = cache
        ops.split_bind(W.detach(), cache[1], mode, n_attrs)

    def embed_segments(self, segs, ld_e: int):
        """segs: [(x, a, c, is_target)] -> ([e [B,T,ld_e]], zq).  One fused call for all segments."""
        table = self.attr_table()
        self.bind_split_weights(table.shape[1] if table is not None else segs[0][1].shape[-1])
        pos = _segs_pos(self.enc, segs)
        call = [(x, a, c, (not tgt) and pos is not None) for (x, a, c, tgt) in segs]
        return ops.embed_fwd(call, self.items_embed.weight, self.feats_embed.weight, self.feats_embed.bias,
                             self.joint_embed.weight, self.joint_embed.bias, pos, ld_e, attrs_table=self.attr_table())

    # ---- opt-in re-association for TRAINING (CARCA.fold_embedding(True, training=True)) -------------------------
    # AllEmbedding is linear (carca.py:86-89): e = sqrt(d) E[x] W_jz^T + [a;c] (W_jq W_f)^T + (W_jq b_f + b_j).  Evaluated in
    # that order the F -> g product never happens: the forward needs one F -> d GEMM (14 instead of 71 GFLOP at C2) and
    # the backward one F -> d weight-gradient product G = (de*mask)^T [a;c], from which
    #   d W_f = W_jq^T G,  d b_f = W_jq^T cs,  d W_jq = G W_f^T + cs (x) b_f,  cs = colsum(de*mask) = d b_j
    # are small products.  Same algebra, different fp32 summation order (~1e-6 relative).
    def _embed_segments_folded(self, segs, ld_e: int):
        d = self.d
        wc, bias_c = self.folded_weights()  # recomposed at every training step (the cache key carries the epoch)
        E, Wj = self.items_embed.weight.detach(), self.joint_embed.weight.detach()
        table = self.attr_table()
        pos = _segs_pos(self.enc, segs)
        n_ctx = segs[0][2].shape[-1]
        n_attrs = table.shape[1] if table is not None else segs[0][1].shape[-1]
        es = [torch.empty(x.shape[0], x.shape[1], ld_e, dtype=torch.float32, device=E.device) for (x, _, _, _) in segs]
        outs = [e.view(-1, ld_e) for e in es]
        ops.gemm_rows([dict(a0=E, a0_gather=True, ids=x, out=o) for (x, _, _, _), o in zip(segs, outs)], Wj[:, :d], d, d,
                      ld_e, bias=bias_c, alpha=float(d) ** 0.5)

        def src(a, x):
            return dict(a0=a) if a is not None else dict(a0=table, a0_gather=True)

        ops.gemm_rows([dict(a1=c if n_ctx else None, ids=x, add=o, out=o, add_pos=(not tgt) and pos is not None,
                            T=x.shape[1], **src(a, x)) for (x, a, c, tgt), o in zip(segs, outs)],
                      wc[:, :n_attrs], d, n_attrs, ld_e, bt1=wc[:, n_attrs:] if n_ctx else None, K1=n_ctx, pos=pos,
                      mask_rows=True)
        return es

    def _embed_backward_folded(self, des, segs, gbp, L: int, dpi: int) -> None:
        d = self.d
        E, Wj, Wf, bf = (p.detach() for p in (self.items_embed.weight, self.joint_embed.weight, self.feats_embed.weight,
                                               self.feats_embed.bias))
        g_feats, F = Wf.shape
        table = self.attr_table()
        n_ctx = segs[0][2].shape[-1]
        n_attrs = F - n_ctx
        ids_seg = [sg[0] for sg in segs]
        nseg = len(des)
        if not segs[0][3]:  # (segment 0 is the profile: the only one with a position term, carca.py:91)
            _pos_grad(self.enc, des[0], ids_seg[0], d, L, gbp)
        g_joint_w, g_joint_b = gbp[id(self.joint_embed.weight)], gbp[id(self.joint_embed.bias)]
        # d W_jz = sqrt(d) (de*mask)^T E[x];  d b_j = cs
        ops.gemm_wgrad([dict(dy=des[i], x=E, x_gather=True, ids=ids_seg[i]) for i in range(nseg)], d, d, g_joint_w[:, :d],
                       g_joint_b, mask_rows=True)
        g_joint_w[:, :d].mul_(float(d) ** 0.5)
        # d E[x] += sqrt(d) (de*mask) W_jz
        wjz_t = ops.PackedWeights([ops.PackItem(Wj[:, :d], d, dpi, transposed=True)], des[0].device)
        wjz_t.pack()
        dz = ops.gemm_rows([dict(a0=des[i], ids=ids_seg[i]) for i in range(nseg)], wjz_t.view(0), d, d, d, mask_rows=True)
        g_items = gbp[id(self.items_embed.weight)]
        for i in range(nseg):
            ops.embed_scatter(dz[i], ids_seg[i], d, float(d) ** 0.5, g_items)
        # G = (de*mask)^T [a ; c]   [d, F]
        G = torch.zeros(d, F, dtype=torch.float32, device=des[0].device)

        def xsrc(i):
            a = segs[i][1]
            return dict(x=a) if a is not None else dict(x=table, x_gather=True)

        ops.gemm_wgrad([dict(dy=des[i], ids=ids_seg[i], x1=segs[i][2] if n_ctx else None, **xsrc(i)) for i in range(nseg)],
                       d, n_attrs, G, None, mask_rows=True, K1=n_ctx)
        wjq = Wj[:, d:]  # [d, g] view
        cs = g_joint_b    # colsum(de*mask), complete in stream order
        ops.gemm_wgrad([dict(dy=wjq, x=G)], g_feats, F, gbp[id(self.feats_embed.weight)], None)
        ops.gemm_wgrad([dict(dy=wjq, x=cs.view(d, 1))], g_feats, 1, gbp[id(self.feats_embed.bias)].view(g_feats, 1), None)
        # d W_jq = G W_f^T + cs (x) b_f: 90 rows against K = 4102 is one long dependent chain per block as a row GEMM (150 us),
        # so it runs as a weight-gradient product over the F "rows" of the two transposed operands instead
        g_t = ops.PackedWeights([ops.PackItem(G, F, dpi, transposed=True)], G.device)  # G^T [F, dpi]
        g_t.pack()
        wf_t = self.__dict__["_wf_t"].view(0)                                          # W_f^T [F, g] of this step's forward
        ops.gemm_wgrad([dict(dy=g_t.view(0), x=wf_t)], d, g_feats, g_joint_w[:, d:], None)
        g_joint_w[:, d:].addmm_(cs.view(d, 1), bf.view(1, g_feats))

    def late_grad_params(self, saved):
        """The parameters whose gradient the backward's LAST launch produces (autograd._grad_buffers lays them out behind
        the others so that a sharded step can reduce everything else under that launch)."""
        return () if isinstance(saved, str) else (self.feats_embed.weight, self.feats_embed.bias)

    def side_grad_params(self):
        """The dense parameters embed_backward accumulates into with a read-modify-write at the end of a kernel: a second,
        concurrent embed_backward call of the same pass (autograd._SideEmbed) needs buffers of its own for them.  (The
        item table's rows are scatter-added with atomics: shared; d joint_embed stays in one call over all rows.)"""
        return (self.feats_embed.weight, self.feats_embed.bias)

    def backward_pack_items(self, dpi: int):
        """The transposed weight copy embed_backward needs (Bt[n = input feature of joint_embed][k = output feature]): the
        backward pass packs it in ITS pack launch and hands the view back as embed_backward(..., wj_t=)."""
        return [ops.PackItem(self.joint_embed.weight, self.d + self.feats_embed.weight.shape[0], dpi, transposed=True)]

    def embed_backward(self, des, segs, zq, gbp, L: int, dpi: int, wj_t=None, joint_only=None, skip_joint=False) -> None:
        """Backward of embed_segments (carca.py:85-95): des[i] = d e of segment i, [rows, dpi], NOT yet masked;
        accumulates into the gradient buffers gbp[id(param)].  One host call (carca_embed_bwd): position-encoding
        gradient, d joint_embed, d [z ; q], item-row scatter-add, d feats_embed.  joint_only / skip_joint: see
        autograd._SideEmbed (the target rows' share on a second stream)."""
        if isinstance(zq, str):  # the forward took the re-associated path
            return self._embed_backward_folded(des, segs, gbp, L, dpi)
        d = self.d
        g_feats = self.feats_embed.weight.shape[0]
        table = self.attr_table()
        n_attrs = table.shape[1] if table is not None else segs[0][1].shape[-1]
        n_ctx = segs[0][2].shape[-1]
        if wj_t is None:  # (a caller without a pack plan: own copy, own launch)
            pw = self.__dict__.get("_wj_t")  # Bt[n = input feature of joint_embed][k = output feature]: repacked every step
            if pw is None or pw.buf.device != des[0].device or pw.items[0].dst_cols != dpi:
                pw = ops.PackedWeights(self.backward_pack_items(dpi), des[0].device)
                self.__dict__["_wj_t"] = pw
            pw.items[0].src = self.joint_embed.weight
            pw.pack()
            wj_t = pw.view(0)
        enc_w = self.enc.encoding.weight if hasattr(self.enc, "encoding") else None
        ops.embed_bwd(des, segs, zq, wj_t,
                      dict(g_items=gbp[id(self.items_embed.weight)], g_feats_w=gbp[id(self.feats_embed.weight)],
                           g_feats_b=gbp[id(self.feats_embed.bias)], g_joint_w=gbp[id(self.joint_embed.weight)],
                           g_joint_b=gbp[id(self.joint_embed.bias)]),
                      table, d, g_feats, n_attrs, n_ctx, L,
                      gbp[id(enc_w)] if (enc_w is not None and not segs[0][3]) else None,  # (targets carry no position term)
                      joint_only=joint_only, skip_joint=skip_joint)

    def _embed_unmasked(self, x: Tensor, a: Optional[Tensor], c: Tensor, target: bool) -> Tensor:
        """carca.py:86-92 WITHOUT line 94: W_j [sqrt(d) E[x] ; W_f [a;c] + b_f] + b_j (+ position term) for every slot, id 0
        included (E[0] is the zero row of padding_idx = 0, carca.py:73) -- what a caller-supplied mask that keeps a slot
        whose id is 0 multiplies.  Three row GEMMs; inference only."""
        d, E = self.d, self.items_embed.weight.detach()
        Wf, bf, Wj, bj = (p.detach() for p in (self.feats_embed.weight, self.feats_embed.bias, self.joint_embed.weight,
                                               self.joint_embed.bias))
        g = Wf.shape[0]
        table = self.attr_table()
        n_ctx = c.shape[-1]
        n_attrs = table.shape[1] if table is not None else a.shape[-1]
        pos = None if target else _position_table(self.enc, x.shape[1])
        ids = ops._ids32(x.reshape(-1))
        src = dict(a0=ops._f32(a).reshape(-1, n_attrs)) if a is not None else dict(a0=table, a0_gather=True, ids=ids)
        (q,) = ops.gemm_rows([dict(a1=ops._f32(c).reshape(-1, n_ctx) if n_ctx else None, **src)], Wf[:, :n_attrs], g, n_attrs,
                             (g + 3) // 4 * 4, bt1=Wf[:, n_attrs:] if n_ctx else None, K1=n_ctx, bias=bf)
        e = torch.empty(x.shape[0], x.shape[1], d, dtype=torch.float32, device=E.device)
        o = e.view(-1, d)
        ops.gemm_rows([dict(a0=E, a0_gather=True, ids=ids, out=o)], Wj[:, :d], d, d, d, bias=bj, alpha=float(d) ** 0.5)
        ops.gemm_rows([dict(a0=q, ids=ids, add=o, out=o, add_pos=pos is not None, T=x.shape[1])], Wj[:, d:], d, g, d, pos=pos)
        return e

    def forward(self, x: Tensor, a: Tensor, c: Tensor, mask: Tensor, target: bool) -> Tensor:
        """abstract.py:22 / carca.py:85-95.  The fused kernels take the mask as x != 0 -- what get_mask(x) is at every call
        site of the reference (carca.py:413-426).  Any OTHER mask is honoured as carca.py:94 does (`e * mask.unsqueeze(2)`):
        see _apply_caller_mask."""
        return _apply_caller_mask(self, x, a, c, mask, target)


# ------------------------------------------------------------------------------------------------
# ablation variants (carca.py:98-198, 352-399) -- SURVEY.md section 8 row f4.  Same constructors and state_dict as
# the reference; the embeddings are AllEmbedding's row GEMM with terms removed, the decoders a row-dot epilogue of
# the final LayerNorm.  Each class brings the two halves the engine calls:
#   embeddings: embed_segments(segs, ld_e) -> (es, saved) and embed_backward(des, segs, saved, gbp, L, dpi)
#   decoders:   score_groups(p, os, B, L, d, dpi) -> (ys, saved) and score_backward(dys, saved, ...) -> (dp, d os)
# ------------------------------------------------------------------------------------------------
def _standalone_embed(module, x, a, c, target):
    if torch.is_grad_enabled() and any(p.requires_grad for p in module.parameters()):
        from .autograd import embed_with_grad

        return embed_with_grad(module, x, a, c, target)
    (e,), _ = module.embed_segments([(x, a, c, target)], ld_e=module.d)
    return e


def _apply_caller_mask(module, x, a, c, mask, target):
    """Embedding.forward(x, a, c, mask, target) of the ABC (abstract.py:22) with the caller's `mask` honoured
    (carca.py:94,120,149,166,197: `e * mask.unsqueeze(2)`).  The kernels mask with x != 0; so
      * mask is None or equals get_mask(x) (every call of the reference): the fused path as it is;
      * mask is zero wherever x is 0 (it drops or re-weights valid slots): the fused result times the mask -- exact, and
        differentiable like the reference's multiply;
      * mask keeps a slot whose id is 0: the reference embeds that slot (item row 0 + its attributes / context) and scales
        it; AllEmbedding runs its unmasked row products and multiplies (inference); with gradients enabled, or for the
        ablation embeddings, this raises instead of returning another answer than the reference's.
    Stand-alone module surface only (CARCA.forward builds its masks itself): the comparison costs one host read."""
    if mask is None:
        return _standalone_embed(module, x, a, c, target)
    ops._need_cuda(x, mask)
    if mask.shape != x.shape:
        raise ValueError(f"mask {tuple(mask.shape)} must have the shape of the ids {tuple(x.shape)}")
    valid = x != 0
    m = mask.to(torch.float32)
    flags = torch.stack([(m == valid.to(torch.float32)).all(), (m[~valid] == 0).all()]).tolist()  # (one host read)
    if flags[0]:
        return _standalone_embed(module, x, a, c, target)
    if flags[1]:
        return _standalone_embed(module, x, a, c, target) * m.unsqueeze(2)
    grad = torch.is_grad_enabled() and any(p.requires_grad for p in module.parameters())
    if grad or not hasattr(module, "_embed_unmasked"):
        raise CarcaHipError(f"{type(module).__name__}.forward: `mask` keeps slots whose id is 0; the fused kernels leave those "
                            "rows out (x != 0) -- supported for AllEmbedding under torch.no_grad() only")
    return module._embed_unmasked(x, a, c, target) * m.unsqueeze(2)


class _FeatsEmbedding(Embedding):
    """AttrCtxEmbedding / AttrEmbedding: e = (W_j (W_f [a(;c)] + b_f) + b_j (+pos)) * mask  (carca.py:112-121,141-150)."""
    _use_ctx = True

    def _build(self, d: int, g: int, n_in: int, enc: Encoding):
        self.d, self.enc = d, enc
        self.feats_embed = nn.Linear(in_features=n_in, out_features=g)
        self.joint_embed = nn.Linear(in_features=g, out_features=d)
        for m in (self.feats_embed, self.joint_embed):
            nn.init.xavier_uniform_(m.weight)
        for m in (self.feats_embed, self.joint_embed):
            nn.init.zeros_(m.bias)

    def __getstate__(self):
        state = dict(super().__getstate__())
        state.pop("_attr_table", None)
        return _drop_tables(state)

    def register_attr_table(self, attrs: Optional[Tensor]) -> None:
        """As AllEmbedding.register_attr_table: the [n_items, n_attrs] item-attribute matrix on the device; afterwards
        `a` may be None (rows gathered by id).  Pass None to unregister."""
        if attrs is None:
            self.__dict__.pop("_attr_table", None)
            return
        n_ctx_max = self.feats_embed.in_features
        if attrs.dim() != 2 or attrs.shape[1] > n_ctx_max:
            raise CarcaHipError("register_attr_table: expected [n_items, n_attrs] with n_attrs <= feats_embed.in_features")
        self.__dict__["_attr_table"] = attrs.detach().to(self.feats_embed.weight.device, torch.float32).contiguous()

    def attr_table(self) -> Optional[Tensor]:
        return self.__dict__.get("_attr_table")

    def item_table(self) -> Tensor:
        """T [n_items, row_ld(d)] = e(i, c = 0) for every item of the registered attribute table."""
        table = _need_attr_table(self, "item_table")
        n_ctx = self.feats_embed.in_features - table.shape[1] if self._use_ctx else 0
        return _cached_table(self, "_item_table_cache", cached_parameters(self), (id(table),), lambda: _target_table(
            self, table.shape[0], table.view(1, table.shape[0], table.shape[1]), n_ctx, table.device), keep=table)

    def context_matrix(self, n_ctx: int) -> Optional[Tensor]:
        """M [d, n_ctx] = W_j W_f[:, n_attrs:] for AttrCtxEmbedding (carca.py:113-114); None for AttrEmbedding."""
        if n_ctx == 0 or not self._use_ctx:
            return None
        Wf, Wj = self.feats_embed.weight, self.joint_embed.weight

        def build():
            F, g = Wf.shape[1], Wf.shape[0]
            wf_ctx_t = Wf.detach()[:, F - n_ctx:].t().contiguous()  # [n_ctx, g] (data movement)
            (m,) = ops.gemm_rows([dict(a0=Wj.detach())], wf_ctx_t, n_ctx, g, (n_ctx + 3) // 4 * 4)
            return m[:, :n_ctx]
        return _cached_table(self, "_ctx_matrix_cache", (Wf, Wj), (n_ctx,), build)

    def _split(self, segs):
        n_ctx = segs[0][2].shape[-1] if self._use_ctx else 0
        n_attrs = self.feats_embed.in_features - n_ctx
        return n_attrs, n_ctx

    def embed_segments(self, segs, ld_e: int):
        d, Wf, Wj = self.d, self.feats_embed.weight, self.joint_embed.weight
        g = Wf.shape[0]
        n_attrs, n_ctx = self._split(segs)
        g_ld = (g + 3) // 4 * 4
        pos = _segs_pos(self.enc, segs)
        table = self.attr_table()

        def src(x, a):  # a None: the rows of the registered attribute table, gathered by id inside the product
            if a is not None:
                return dict(a0=a)
            if table is None:
                raise CarcaHipError(f"{type(self).__name__}: attrs is None and no attribute table is registered "
                                    "(register_attr_table)")
            return dict(a0=table, a0_gather=True, ids=x)
        qs = ops.gemm_rows([dict(a1=c if n_ctx else None, **src(x, a)) for (x, a, c, _) in segs], Wf[:, :n_attrs], g,
                           n_attrs, g_ld, bt1=Wf[:, n_attrs:] if n_ctx else None, K1=n_ctx, bias=self.feats_embed.bias)
        es = ops.gemm_rows([dict(a0=qs[i], ids=x, T=x.shape[1], add_pos=(not tgt) and pos is not None)
                            for i, (x, _, _, tgt) in enumerate(segs)], Wj, d, g, ld_e, bias=self.joint_embed.bias,
                           pos=pos, mask_rows=True)
        return [e.view(x.shape[0], x.shape[1], ld_e) for e, (x, _, _, _) in zip(es, segs)], qs

    def embed_backward(self, des, segs, qs, gbp, L: int, dpi: int) -> None:
        d, Wf, Wj = self.d, self.feats_embed.weight, self.joint_embed.weight
        g = Wf.shape[0]
        n_attrs, n_ctx = self._split(segs)
        ids_seg = [sg[0] for sg in segs]
        nseg = len(des)
        if not segs[0][3]:  # (a target segment carries no position term)
            _pos_grad(self.enc, des[0], ids_seg[0], d, L, gbp)
        ops.gemm_wgrad([dict(dy=des[i], x=qs[i], ids=ids_seg[i]) for i in range(nseg)], d, g, gbp[id(Wj)],
                       gbp[id(self.joint_embed.bias)], mask_rows=True)
        wj_t = ops.PackedWeights([ops.PackItem(Wj, g, dpi, transposed=True)], des[0].device)
        wj_t.pack()
        dqs = ops.gemm_rows([dict(a0=des[i], ids=ids_seg[i]) for i in range(nseg)], wj_t.view(0), g, d, g,
                            mask_rows=True)
        ops.gemm_wgrad([dict(dy=dqs[i], x=segs[i][1], x1=segs[i][2] if n_ctx else None) for i in range(nseg)], g,
                       n_attrs, gbp[id(Wf)], gbp[id(self.feats_embed.bias)], K1=n_ctx)

    def forward(self, x, a, c, mask, target):
        return _apply_caller_mask(self, x, a, c, mask, target)


class AttrCtxEmbedding(_FeatsEmbedding):
    def __init__(self, d: int, g: int, n_ctx: int, n_attrs: int, enc: Encoding):
        super().__init__()
        self._build(d, g, n_ctx + n_attrs, enc)


class AttrEmbedding(_FeatsEmbedding):
    _use_ctx = False

    def __init__(self, d: int, g: int, n_attrs: int, enc: Encoding):
        super().__init__()
        self._build(d, g, n_attrs, enc)


class IdEmbedding(Embedding):
    """e = (E[x] * sqrt(d) (+pos)) * mask  (carca.py:164-171): the gather rides a d x d row GEMM against sqrt(d) I, whose
    single non-zero term per output reproduces the reference's one rounding exactly."""

    def __init__(self, n_items: int, d: int, enc: Encoding):
        super().__init__()
        self.d, self.enc = d, enc
        self.items_embed = nn.Embedding(num_embeddings=n_items, embedding_dim=d, padding_idx=0)
        nn.init.xavier_uniform_(self.items_embed.weight)
        with torch.no_grad():
            self.items_embed.weight[0].zero_()

    def _scaled_identity(self, device) -> Tensor:
        eye = self.__dict__.get("_eye")
        if eye is None or eye.device != device:
            eye = torch.eye(self.d, dtype=torch.float32, device=device) * (float(self.d) ** 0.5)
            self.__dict__["_eye"] = eye
        return eye

    def __getstate__(self):
        state = dict(super().__getstate__())
        state.pop("_eye", None)
        return _drop_tables(state)

    def item_table(self) -> Tensor:
        """T [n_items, row_ld(d)] = sqrt(d) E (row 0 = 0); the embedding ignores context."""
        E = self.items_embed.weight
        return _cached_table(self, "_item_table_cache", (E,), (), lambda: _target_table(self, E.shape[0], None, 0, E.device))

    def context_matrix(self, n_ctx: int) -> Optional[Tensor]:
        return None

    def embed_segments(self, segs, ld_e: int):
        d, E = self.d, self.items_embed.weight
        pos = _segs_pos(self.enc, segs)
        es = ops.gemm_rows([dict(a0=E, a0_gather=True, ids=x, T=x.shape[1], add_pos=(not tgt) and pos is not None)
                            for (x, _, _, tgt) in segs], self._scaled_identity(E.device), d, d, ld_e, pos=pos,
                           mask_rows=True)
        return [e.view(x.shape[0], x.shape[1], ld_e) for e, (x, _, _, _) in zip(es, segs)], None

    def embed_backward(self, des, segs, saved, gbp, L: int, dpi: int) -> None:
        d = self.d
        ids_seg = [sg[0] for sg in segs]
        if not segs[0][3]:  # (a target segment carries no position term)
            _pos_grad(self.enc, des[0], ids_seg[0], d, L, gbp)
        for i in range(len(des)):  # rows with id 0 are skipped: that is the e * mask of carca.py:170
            ops.embed_scatter(des[i], ids_seg[i], d, float(d) ** 0.5, gbp[id(self.items_embed.weight)])

    def forward(self, x, a, c, mask, target):
        return _apply_caller_mask(self, x, a, c, mask, target)


class MLPIdEmbedding(Embedding):
    """e = (W (E[x] * sqrt(d)) + b (+pos)) * mask with a g-wide item table (carca.py:190-198)."""

    def __init__(self, n_items: int, d: int, g: int, enc: Encoding):
        super().__init__()
        self.d, self.enc = d, enc
        self.items_embed = nn.Embedding(num_embeddings=n_items, embedding_dim=g, padding_idx=0)
        self.feats_embed = nn.Linear(in_features=g, out_features=d)
        nn.init.xavier_uniform_(self.items_embed.weight)
        nn.init.xavier_uniform_(self.feats_embed.weight)
        nn.init.zeros_(self.feats_embed.bias)
        with torch.no_grad():
            self.items_embed.weight[0].zero_()

    def __getstate__(self):
        return _drop_tables(dict(super().__getstate__()))

    def item_table(self) -> Tensor:
        """T [n_items, row_ld(d)] = W sqrt(d) E[i] + b for i != 0, row 0 = 0; the embedding ignores context."""
        E = self.items_embed.weight
        return _cached_table(self, "_item_table_cache", cached_parameters(self), (),
                             lambda: _target_table(self, E.shape[0], None, 0, E.device))

    def context_matrix(self, n_ctx: int) -> Optional[Tensor]:
        return None

    def embed_segments(self, segs, ld_e: int):
        d, E, W = self.d, self.items_embed.weight, self.feats_embed.weight
        g = E.shape[1]
        pos = _segs_pos(self.enc, segs)
        es = ops.gemm_rows([dict(a0=E, a0_gather=True, ids=x, T=x.shape[1], add_pos=(not tgt) and pos is not None)
                            for (x, _, _, tgt) in segs], W, d, g, ld_e, bias=self.feats_embed.bias, pos=pos,
                           mask_rows=True, alpha=float(d) ** 0.5)
        return [e.view(x.shape[0], x.shape[1], ld_e) for e, (x, _, _, _) in zip(es, segs)], None

    def embed_backward(self, des, segs, saved, gbp, L: int, dpi: int) -> None:
        d, E, W = self.d, self.items_embed.weight, self.feats_embed.weight
        g = E.shape[1]
        sd = float(d) ** 0.5
        ids_seg = [sg[0] for sg in segs]
        nseg = len(des)
        if not segs[0][3]:  # (a target segment carries no position term)
            _pos_grad(self.enc, des[0], ids_seg[0], d, L, gbp)
        # d W = sqrt(d) (d e * mask)^T E[x]; the table rows are gathered inside the product
        gw = torch.zeros_like(gbp[id(W)])
        ops.gemm_wgrad([dict(dy=des[i], x=E.detach(), x_gather=True, ids=ids_seg[i]) for i in range(nseg)], d, g, gw,
                       gbp[id(self.feats_embed.bias)], mask_rows=True)
        gbp[id(W)].add_(gw, alpha=sd)
        w_t = ops.PackedWeights([ops.PackItem(W, g, dpi, transposed=True)], des[0].device)
        w_t.pack()
        dzs = ops.gemm_rows([dict(a0=des[i], ids=ids_seg[i]) for i in range(nseg)], w_t.view(0), g, d, g,
                            mask_rows=True)
        for i in range(nseg):
            ops.embed_scatter(dzs[i], ids_seg[i], g, sd, gbp[id(E)])

    def forward(self, x, a, c, mask, target):
        return _apply_caller_mask(self, x, a, c, mask, target)


class _DotDecoder(Decoder):
    """Row-dot decoders over the final-normed profile (carca.py:352-399).  Neither looks at the masks."""

    def _standalone(self, o, p):
        if torch.is_grad_enabled() and (o.requires_grad or p.requires_grad):
            raise CarcaHipError(f"training through a stand-alone {type(self).__name__} is not built; train through "
                                f"CARCA.forward")
        B, L, d = p.shape
        ys, _ = self.score_groups(p.reshape(B * L, d), [o.reshape(-1, d)], [o.shape[1]], B, L, d, d)
        return ys[0]


class DotProduct(_DotDecoder):
    def __init__(self) -> None:
        super().__init__()
        self.sig = nn.Sigmoid()

    def score_groups(self, p2d: Tensor, os2d: List[Tensor], Ts: List[int], B: int, L: int, d: int, dpi: int):
        """y_g = sigmoid(p . o): slot t against target t in train mode, last slot against all in eval (carca.py:361-367)."""
        slot = self.training
        ys = [ops.dot_score_fwd(p2d, o, B, L, T, d, slot, 0) for o, T in zip(os2d, Ts)]
        return ys, dict(p=p2d, os=os2d, Ts=Ts, ys=ys, slot=slot)

    def score_backward(self, dys, sv, B: int, L: int, d: int, dpi: int):
        dp = torch.zeros(B * L, dpi, dtype=torch.float32, device=sv["p"].device)
        dos = [ops.dot_score_bwd(sv["p"], o, y, dy, dp, B, L, T, d, sv["slot"], 0, dpi)
               for o, y, dy, T in zip(sv["os"], sv["ys"], dys, sv["Ts"])]
        return dp, dos

    def forward(self, o, o_mask, p, p_mask):
        return self._standalone(o, p)


class WeightedDotProduct(_DotDecoder):
    def __init__(self, gamma: float, seq_len: int, normalize: bool, device: str):
        super().__init__()
        self.norm = normalize
        self.gamma = float(gamma)
        self.W = (gamma ** torch.arange(0, seq_len, device=device).unsqueeze(0).repeat(seq_len, 1)).tril().unsqueeze(-1)
        self.sig = nn.Sigmoid()

    def score_groups(self, p2d: Tensor, os2d: List[Tensor], Ts: List[int], B: int, L: int, d: int, dpi: int):
        """p' = p[t] * sum_{j<=t} gamma^j (what the reference's repeat / tril / sum does, carca.py:385-386); optional L2
        normalisation of p' and o; y = sigmoid(p' . o) or (p' . o + 1) / 2 (carca.py:388-397)."""
        slot = self.training
        ld = max(dpi, d)
        pw = ops.slot_decay_scale(p2d, B, L, d, self.gamma, ld)
        if self.norm:
            pq = ops.l2norm_fwd(pw, d, ld)
            oq = [ops.l2norm_fwd(o, d, ld) for o in os2d]
        else:
            pq, oq = pw, os2d
        link = 1 if self.norm else 0
        ys = [ops.dot_score_fwd(pq, o, B, L, T, d, slot, link) for o, T in zip(oq, Ts)]
        return ys, dict(pw=pw, pq=pq, os=os2d, oq=oq, Ts=Ts, ys=ys, slot=slot, link=link)

    def score_backward(self, dys, sv, B: int, L: int, d: int, dpi: int):
        dpq = torch.zeros(B * L, dpi, dtype=torch.float32, device=sv["pq"].device)
        doq = [ops.dot_score_bwd(sv["pq"], o, y, dy, dpq, B, L, T, d, sv["slot"], sv["link"], dpi)
               for o, y, dy, T in zip(sv["oq"], sv["ys"], dys, sv["Ts"])]
        if self.norm:
            dpw = ops.l2norm_bwd(sv["pw"], dpq, d, dpi)
            dos = [ops.l2norm_bwd(o, g, d, dpi) for o, g in zip(sv["os"], doq)]
        else:
            dpw, dos = dpq, doq
        return ops.slot_decay_scale(dpw, B, L, d, self.gamma, dpi), dos  # the slot weights are diagonal: own transpose

    def forward(self, o, o_mask, p, p_mask):
        return self._standalone(o, p)


# ------------------------------------------------------------------------------------------------
# attention (carca.py:204-349)
# ------------------------------------------------------------------------------------------------


class MultiHeadAttention(nn.Module):
    """Parameter holder with the reference's names (carca.py:204-226).

    Its arithmetic (carca.py:228-265) runs fused inside SelfAttentionBlock / CrossAttentionBlock.
    """

    def __init__(self, embed_dim: int, num_heads: int, dropout: float):
        super().__init__()
        assert embed_dim % num_heads == 0.0, "Embedding dim must be divisible by number of heads"
        self.d = embed_dim
        self.H = num_heads
        self.WQ = nn.Linear(in_features=embed_dim, out_features=embed_dim)
        self.WK = nn.Linear(in_features=embed_dim, out_features=embed_dim)
        self.WV = nn.Linear(in_features=embed_dim, out_features=embed_dim)
        self.softmax = nn.Softmax(dim=-1)
        self.dropout = nn.Dropout(p=dropout)
        for m in (self.WQ, self.WK, self.WV):
            nn.init.xavier_uniform_(m.weight)
        for m in (self.WQ, self.WK, self.WV):
            nn.init.zeros_(m.bias)

    def pack_items(self, dpi: int, dhp: int, dpo: int) -> List[ops.PackItem]:
        dh = self.d // self.H
        mats = [ops.PackItem(m.weight, dpo, dpi, row_heads=(dh, dhp), frag16=True) for m in (self.WQ, self.WK, self.WV)]
        vecs = [ops.PackItem(m.bias, 1, dpo, col_heads=(dh, dhp)) for m in (self.WQ, self.WK, self.WV)]
        return mats + vecs

    def forward(self, query, key, value, q_mask, k_mask, causal: int = None, return_w: bool = False):
        """Stand-alone MultiHeadAttention.forward (carca.py:228-265): three row GEMMs for the projections and
        carca_mha_core for the attention (the blocks' fused kernels never come here).  Returns the merged heads
        [B, Tq, d], or (weights [H*B, Tq, Tk] before dropout, output) with return_w -- the reference's order.
        Differentiable (autograd.mha_with_grad: carca_mha_core_bwd + row / weight-gradient GEMMs).
        Train mode with p > 0 (carca.py:258, self.dropout on the weights): the masks are drawn inside carca_mha_core_drop
        from a seed taken from torch's CPU generator (torch's Philox stream cannot be reproduced in a kernel); the keep-mask
        of the last call, uint8 [B, H, Tq, Tk], stays on the module as `last_keep_mask` for replay (tests/test_hip_dropout.py)."""
        ops._need_cuda(query, key, value, q_mask, k_mask)
        drop = None
        self.__dict__["last_keep_mask"] = None
        if self.training and self.dropout.p > 0:
            if self.dropout.p >= 1:
                raise CarcaHipError("MultiHeadAttention: dropout p must be < 1")
            drop = (float(self.dropout.p), ops.new_dropout_seed(), 0)
        if torch.is_grad_enabled() and (any(t.requires_grad for t in (query, key, value)) or
                                        any(p.requires_grad for p in self.parameters())):
            from .autograd import mha_with_grad

            return mha_with_grad(self, query, key, value, q_mask, k_mask, causal, return_w, drop=drop)
        d = self.d
        proj = []
        for x, lin in ((query, self.WQ), (key, self.WK), (value, self.WV)):
            x2 = ops._f32(x).reshape(-1, x.shape[-1])
            (y,) = ops.gemm_rows([dict(a0=x2)], lin.weight.detach(), d, d, d, bias=lin.bias.detach())
            proj.append(y.view(x.shape[0], x.shape[1], d))
        res = ops.mha_core(proj[0], proj[1], proj[2], q_mask != 0, k_mask != 0, self.H, causal, return_w, drop=drop)
        out, w = res[0], res[1]
        if len(res) == 3:
            self.__dict__["last_keep_mask"] = res[2]
        return (w, out) if return_w else out


# Packed / composed weight caches are keyed on (data_ptr, _version) of their parameters -- but not every optimizer bumps
# _version (torch.optim.Adam(fused=True) updates parameters without touching it), so the key also carries an epoch
# that every training-mode forward advances: a training forward always repacks (weights change every step anyway) and
# the first inference forward after training repacks once; inference loops keep their caches.
_WEIGHT_EPOCH = [0]
USE_Z_TABLE = True  # inference: the joint embedding's item term from AllEmbedding.z_table() (False: gather + d + g columns; A/B)


def note_training_forward() -> None:
    _WEIGHT_EPOCH[0] += 1


def cached_parameters(module: nn.Module) -> List[nn.Parameter]:
    """list(module.parameters()) without walking the module tree on every call (0.25 ms per train step at C2).
    The cached list is revalidated against the tree it was built from -- every _parameters / _modules dict of the
    subtree must still hold the same objects -- so replacing a parameter or a sub-module is picked up."""
    c = module.__dict__.get("_param_cache")
    if c is not None:
        sizes, checks, params = c
        if all(len(d) == n for d, n in sizes) and all(d.get(k) is o for d, k, o in checks):
            return params
    sizes, checks = [], []
    for m in module.modules():
        for d in (m._parameters, m._modules):
            sizes.append((d, len(d)))
            checks.extend((d, k, o) for k, o in d.items())
    params = list(module.parameters())
    module.__dict__["_param_cache"] = (sizes, checks, params)
    return params


class _PackedModule:
    """Mixin: (re)packs this module's parameters into the kernels' layout when any of them changed."""

    def _packed(self, items_fn, device, defer: Optional[list] = None) -> ops.PackedWeights:
        """defer: a list the caller flushes with ops.pack_many (several modules, one launch); None = pack now."""
        key = ((_WEIGHT_EPOCH[0],) + tuple((p.data_ptr(), p._version) for p in self._pack_params()), self._pack_shape(),
               str(device))
        cache = self.__dict__.get("_pack_cache")
        if cache is not None and cache[0] == key:
            return cache[1]
        if cache is not None and cache[0][1:] == key[1:]:
            pw = cache[1]  # same geometry: refill the same device buffer
            pw.items = items_fn()
        else:
            pw = ops.PackedWeights(items_fn(), device)
        if defer is None:
            pw.pack()
        else:
            defer.append(pw)
        self.__dict__["_pack_cache"] = (key, pw)
        return pw

    def __getstate__(self):  # torch.save(model) pickles whole modules (train.py:124): drop the ctypes caches
        state = dict(super().__getstate__())
        for k in ("_pack_cache", "_final_norm_params", "_plan", "_fold_cache", "_param_cache", "_split_cache"):
            state.pop(k, None)
        return _drop_tables(state)


class SelfAttentionBlock(_PackedModule, Encoder):
    def __init__(self, d: int, H: int, p: float, residual: bool):
        super().__init__()
        self.residual = residual
        self.norm1 = nn.LayerNorm(normalized_shape=d)
        self.attn = MultiHeadAttention(embed_dim=d, num_heads=H, dropout=p)
        self.norm2 = nn.LayerNorm(normalized_shape=d)
        self.ffn_1 = nn.Conv1d(in_channels=d, out_channels=d, kernel_size=1)
        self.lrelu = nn.LeakyReLU()
        self.dropout1 = nn.Dropout(p=p)
        self.ffn_2 = nn.Conv1d(in_channels=d, out_channels=d, kernel_size=1)
        self.dropout2 = nn.Dropout(p=p)
        nn.init.xavier_uniform_(self.ffn_1.weight)
        nn.init.xavier_uniform_(self.ffn_2.weight)
        nn.init.zeros_(self.ffn_1.bias)
        nn.init.zeros_(self.ffn_2.bias)

    # -- packing -------------------------------------------------------------------------------
    def _pack_params(self):
        return cached_parameters(self)

    def _pack_shape(self):
        return (self.attn.d, self.attn.H)

    def _items(self) -> List[ops.PackItem]:
        d, H = self.attn.d, self.attn.H
        dpi, dhp, dpo = ops.padded_dims(d, H)
        vec = lambda t: ops.PackItem(t, 1, dpi)  # noqa: E731
        return ([vec(self.norm1.weight), vec(self.norm1.bias), vec(self.norm2.weight), vec(self.norm2.bias)]
                + self.attn.pack_items(dpi, dhp, dpo)
                + [ops.PackItem(self.ffn_1.weight[:, :, 0], dpi, dpi, frag16=True),
                   ops.PackItem(self.ffn_2.weight[:, :, 0], dpi, dpi, frag16=True),
                   vec(self.ffn_1.bias), vec(self.ffn_2.bias)])

    def weights_struct(self, device, defer: Optional[list] = None) -> "_lib.SaWeights":
        pw = self._packed(self._items, device, defer)
        w = _lib.SaWeights()
        names = ["ln1_w", "ln1_b", "ln2_w", "ln2_b", "wq", "wk", "wv", "bq", "bk", "bv", "w1", "w2", "b1", "b2"]
        for i, n in enumerate(names):
            setattr(w, n, pw.ptr(i))
        w._keepalive = pw
        return w

    def _check_mode(self):
        ps = {self.attn.dropout.p, self.dropout1.p, self.dropout2.p}
        if self.training and len(ps) != 1:
            raise CarcaHipError("the fused block kernel takes ONE dropout probability for its three sites "
                                "(the reference constructs them all from the same p, carca.py:280,286,289)")

    def drop_p(self) -> float:
        return float(self.attn.dropout.p) if self.training else 0.0

    def forward(self, x: Tensor, mask: Tensor) -> Tensor:
        """x [B, L, >=d], mask [B, L] (0 = pad) -> [B, L, d] (a view of a padded buffer)."""
        self._check_mode()
        if ops.use_composed(self.attn.d, [self.attn.H], x.shape[1]):
            from . import long_profile

            return long_profile.sa_block(self, x[..., : self.attn.d], mask != 0, ops.new_dropout_seed() if self.training else 0)
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            from .autograd import sa_block_with_grad

            return sa_block_with_grad(self, x, mask)
        d = self.attn.d
        p = self.drop_p()
        y = ops.sa_block_fwd(x, mask != 0, self.weights_struct(x.device), d, self.attn.H, self.residual,
                             drop=(p, ops.new_dropout_seed(), 0) if p > 0 else None)
        return y[..., :d]


class CrossAttentionBlock(_PackedModule, Decoder):
    def __init__(self, d: int, H: int, p: float, residual: bool):
        super().__init__()
        self.residual = residual
        self.attn = MultiHeadAttention(embed_dim=d, num_heads=H, dropout=p)
        self.ffn = nn.Linear(in_features=d, out_features=1)
        self.sig = nn.Sigmoid()
        nn.init.xavier_uniform_(self.ffn.weight)
        nn.init.zeros_(self.ffn.bias)

    def _pack_params(self):
        extra = list(self.__dict__.get("_final_norm_params", ()))
        return cached_parameters(self) + extra

    def _pack_shape(self):
        return (self.attn.d, self.attn.H, len(self.__dict__.get("_final_norm_params", ())))

    def _items(self) -> List[ops.PackItem]:
        d, H = self.attn.d, self.attn.H
        dpi, dhp, dpo = ops.padded_dims(d, H)
        dh = d // H
        items = self.attn.pack_items(dpi, dhp, dpo)
        items += [ops.PackItem(self.ffn.weight, 1, dpo, col_heads=(dh, dhp)), ops.PackItem(self.ffn.weight, 1, dpi),
                  ops.PackItem(self.ffn.bias, 1, 4)]
        # decoder.ffn folded into the value projection (CarcaCaWeights.wu / cu): wu[h] = sum_i w[h,i] W_V[h,i,:],
        # cu[h] = sum_i w[h,i] b_V[h,i] -- the inference kernel scores with P . u instead of w . (P V)
        fv = self.ffn.weight.view(-1)
        items += [ops.PackItem(self.attn.WV.weight, 16, dpi, frag16=True, fold_vec=fv, fold_H=H),
                  ops.PackItem(self.attn.WV.bias.view(-1, 1), 16, 1, fold_vec=fv, fold_H=H)]
        for t in self.__dict__.get("_final_norm_params", ()):
            items.append(ops.PackItem(t, 1, dpi))
        return items

    def weights_struct(self, device, final_norm: Optional[nn.LayerNorm], defer: Optional[list] = None) -> "_lib.CaWeights":
        # the final LayerNorm of CARCA (carca.py:421) is fused into this kernel's prologue
        self.__dict__["_final_norm_params"] = (final_norm.weight, final_norm.bias) if final_norm is not None else ()
        pw = self._packed(self._items, device, defer)
        w = _lib.CaWeights()
        for i, n in enumerate(["wq", "wk", "wv", "bq", "bk", "bv", "ffn_w_pad", "ffn_w", "ffn_b"]):
            setattr(w, n, pw.ptr(i))
        w.wu, w.cu = pw.ptr(9), pw.ptr(10)
        if final_norm is not None:
            w.ln_w, w.ln_b = pw.ptr(11), pw.ptr(12)
        else:
            w.ln_w, w.ln_b = None, None
        w._keepalive = pw
        return w

    def _check_mode(self):
        pass

    def drop_p(self) -> float:
        return float(self.attn.dropout.p) if self.training else 0.0

    def recommend_tables(self, T: Tensor):
        """The scorer's per-item tables over an embedding's item table T (CARCA.recommend): QT = T W_Q^T + b_Q
        [n_items, row_ld(d)], wT [n_items, 4] with column 0 = w_ffn . T[i] (the residual's item term, carca.py:344-345),
        and the block-diagonal [H, d] matrix of w_ffn that folds the value projection per head (u_h = w_h . V_h, as
        CarcaCaWeights.wu / cu).  Composed with carca_gemm_rows, cached per weight version and item table."""
        a = self.attn

        def build():
            d, H = a.d, a.H
            dh = d // H
            (qt,) = ops.gemm_rows([dict(a0=T)], a.WQ.weight.detach(), d, d, ops.row_ld(d), bias=a.WQ.bias.detach())
            (wt,) = ops.gemm_rows([dict(a0=T)], self.ffn.weight.detach(), 1, d, 4)
            wd = torch.zeros(H, d, dtype=torch.float32, device=T.device)
            w = self.ffn.weight.detach().view(H, dh)
            for h in range(H):  # (data movement)
                wd[h, h * dh:(h + 1) * dh] = w[h]
            return qt, wt, wd
        return _cached_table(self, "_reco_cache", (a.WQ.weight, a.WQ.bias, self.ffn.weight), (id(T),), build, keep=T)

    def forward(self, o: Tensor, o_mask: Tensor, p: Tensor, p_mask: Tensor) -> Tensor:
        """Standalone decoder call: p is already final-normed (as in carca.py:421-428)."""
        self._check_mode()
        if ops.use_composed(self.attn.d, [self.attn.H], p.shape[1]):
            from . import long_profile

            d = self.attn.d
            return long_profile.cross_block(self, o[..., :d], o_mask != 0, p[..., :d], p_mask != 0,
                                            ops.new_dropout_seed() if self.training else 0).squeeze()
        if torch.is_grad_enabled() and (o.requires_grad or p.requires_grad or
                                        any(q.requires_grad for q in self.parameters())):
            from .autograd import cross_with_grad

            return cross_with_grad(self, o, o_mask, p, p_mask)
        d, H = self.attn.d, self.attn.H
        dpi, _, _ = ops.padded_dims(d, H)
        o_pad = _pad_cols(o, dpi)
        pd = self.drop_p()
        if pd > 0:  # the keep-masks travel with the saved tensors
            (y,), _, _ = ops.cross_score_fwd(p, p_mask != 0, [(o_pad, o_mask != 0)], self.weights_struct(o.device, None),
                                             d, H, self.residual, self.training, save=True,
                                             drop=(pd, ops.new_dropout_seed(), 0))
        else:
            (y,), _ = ops.cross_score_fwd(p, p_mask != 0, [(o_pad, o_mask != 0)], self.weights_struct(o.device, None),
                                          d, H, self.residual, self.training)
        return y.squeeze()  # bare squeeze, as carca.py:346


class JointScores(list):
    """The per-group score tensors of one forward, views of `.joint` [B, sum N] (column blocks in group order)."""
    joint: Optional[Tensor] = None


def _pad_cols(t: Tensor, width: int) -> Tensor:
    """[.., w] -> contiguous [.., width] with zero pad columns (data movement only)."""
    if t.shape[-1] == width and t.is_contiguous():
        return t
    out = t.new_zeros(*t.shape[:-1], width)
    out[..., : t.shape[-1]] = t
    return out


# ------------------------------------------------------------------------------------------------
# CARCA (carca.py:401-431)
# ------------------------------------------------------------------------------------------------


class CARCA(_PackedModule, Model):
    def __init__(self, d: int, p: float, emb: Embedding, enc: Iterable[Encoder], dec: Decoder):
        super().__init__()
        self.embeds = emb
        self.dropout = nn.Dropout(p=p)
        self.encoder = enc
        self.norm = nn.LayerNorm(normalized_shape=d)
        self.decoder = dec

    def _fusable(self) -> bool:
        """The single-call inference path (carca_forward) covers AllEmbedding + SelfAttentionBlocks + CrossAttentionBlock."""
        return (isinstance(self.embeds, AllEmbedding) and isinstance(self.decoder, CrossAttentionBlock)
                and all(isinstance(b, SelfAttentionBlock) for b in self.encoder))

    def _check_built(self) -> None:
        ok_emb = hasattr(self.embeds, "embed_segments")
        ok_dec = isinstance(self.decoder, CrossAttentionBlock) or hasattr(self.decoder, "score_groups")
        if not (ok_emb and ok_dec and all(isinstance(b, SelfAttentionBlock) for b in self.encoder)):
            raise CarcaHipError("CARCA.forward is built for the reference's embeddings (All/AttrCtx/Attr/Id/MLPId), "
                                "SelfAttentionBlock encoders and its decoders (CrossAttentionBlock/DotProduct/"
                                "WeightedDotProduct); there is no ATen fallback for anything else")

    def _check_eval_built(self, what: str) -> None:
        """What every serving call asks first: eval mode (the scores are forward's eval scores) and a built model."""
        if self.training:
            raise CarcaHipError(f"{what}: the model is in training mode; the call scores with eval semantics "
                                "(call model.eval() first)")
        self._check_built()

    def _model_side(self, what: str, profile, context, allow_composed: bool):
        """The thunk a shared catalogue call runs once its own arguments have passed: () -> the ModelSide."""
        return lambda: catalogue.carca_model_side(self, profile, context, what, allow_composed=allow_composed)

    def _model_side_at(self, what: str, single: str, profile, contexts, allow_composed: bool):
        return lambda: catalogue.carca_model_side_at(self, profile, contexts, what, single, allow_composed=allow_composed)

    def _attn_heads(self) -> List[int]:
        """H of every attention module (the fused kernels are built per (d, H) geometry)."""
        hs = [b.attn.H for b in self.encoder]
        return hs + [self.decoder.attn.H] if isinstance(self.decoder, CrossAttentionBlock) else hs

    def _composed(self, profile, targets) -> bool:
        return ops.use_composed(self.embeds.d, self._attn_heads(), profile[0].shape[1], len(targets))

    def _heads(self) -> int:
        if len(self.encoder):
            return self.encoder[0].attn.H
        return self.decoder.attn.H if isinstance(self.decoder, CrossAttentionBlock) else 1

    def forward(self, profile: Tuple[Tensor, Tensor, Tensor], targets: List[Tuple[Tensor, Tensor, Tensor]]) -> Tensor:
        self._check_built()
        needs_grad = torch.is_grad_enabled() and any(p.requires_grad for p in cached_parameters(self))
        if self._composed(profile, targets):
            # longer than the fused kernels' 64 profile slots, more target groups than one fused call takes (carca.py:424),
            # wider than 128 or a head geometry they are not built for: the same arithmetic from the row-level kernels
            from . import long_profile

            ys = long_profile.forward(self, profile, targets)
        elif needs_grad:
            from .autograd import carca_forward_with_grad

            ys = carca_forward_with_grad(self, profile, targets)
        else:
            ys = self.forward_nograd(profile, targets)
        joint = getattr(ys, "joint", None)
        if joint is not None and isinstance(self.decoder, CrossAttentionBlock) and joint.shape[0] > 1 and \
                all(y.shape[1] > 1 for y in ys):
            return joint  # = torch.cat([y.squeeze() for y in ys], -1): no size-1 dimension for the squeeze to drop
        # each group's scores are squeezed the way CrossAttentionBlock does (carca.py:346), then joined (carca.py:431);
        # the dot decoders return [B, T] unsqueezed (carca.py:361-367)
        if isinstance(self.decoder, CrossAttentionBlock):
            ys = [y.squeeze() for y in ys]
        if len(ys) == 1 and not needs_grad:
            return ys[0]  # (torch.cat of one tensor is a copy: the scores were allocated by this call, hand them out as is)
        return torch.cat(ys, dim=-1)

    def fold_embedding(self, on: bool = True, training: bool = False) -> "CARCA":
        """Opt-in shortcut: compose AllEmbedding's two Linear layers into one (include/carca_hip.h,
        CarcaForwardDesc.fold_wc).  Same algebra, ~1e-6 relative fp32 re-association.  Inference only unless
        training=True, which also re-associates the training step (AllEmbedding._embed_segments_folded: no F -> g
        product in the forward or in the backward)."""
        self.__dict__["_fold"] = bool(on)
        if isinstance(self.embeds, AllEmbedding):
            self.embeds.__dict__["_fold_train"] = bool(on) and bool(training)
        return self

    def catalogue_softmax_loss(self, profile: Tuple[Tensor, Optional[Tensor], Tensor], pos: Tensor) -> Tensor:
        """Full-catalogue softmax cross-entropy of a training batch: profile = (p_x, p_a, p_c) as
        forward takes it, pos = o_x[:, :L] (the positive half of the batch).  Scalar mean over the valid slots (pos in
        [1, n_items)) of logsumexp over every item i >= 1 of the dot decoder's logit minus the positive's logit;
        differentiable in every parameter.  Dot decoders only (WeightedDotProduct without normalisation); attribute-reading
        embeddings need register_attr_table.  Dropout follows self.training, at the sites and with the masks of forward."""
        from .catalogue_xent import catalogue_softmax_loss

        return catalogue_softmax_loss(self, profile, pos)

    def log_prob_rows(self, profile: Tuple[Tensor, Optional[Tensor], Tensor], items: Tensor, temperature: float = 1.0,
                      exclude=None, with_entropy: bool = False,
                      last_slot_only: bool = False) -> Tuple[Tensor, Tensor, Optional[Tensor]]:
        """The policy's log-probabilities as a differentiable quantity: what training on a bandit
        log needs.  -> (log_probs [B, L] float32, valid [B, L] bool, entropy [B, L] float32 or None); log_probs and entropy
        are differentiable in every parameter.

        items has p_x's shape: row (b, t) is the policy "after slot t", softmax(logit / temperature) over its eligible
        items, and log_probs[b, t] the log-probability of items[b, t] under it.  exclude: None, "profile" (row (b, t)
        excludes the non-zero ids of p_x[b, :t + 1]; at t = L - 1 recommend(exclude="profile")'s rule) or an int
        [B, L, E] tensor of ids (0 = padding).  Item i is eligible iff 1 <= i < n_items and not excluded; a row is valid
        iff its own slot is not padding and its action is eligible; log_probs and entropy are exactly 0 on the other rows,
        which get no gradient.  The context cancels in the softmax (section 13), so the value at t = L - 1 is what
        log_prob_items reports for that policy under any request context.  last_slot_only=True reads column L - 1 of
        items (and of an exclude tensor) alone and calls every other row not valid: the bandit shape, one action per user
        after the whole profile, at the cost of B rows instead of B L.  Dot decoders only, as catalogue_softmax_loss;
        dropout follows self.training."""
        from .catalogue_xent import log_prob_rows

        return log_prob_rows(self, profile, items, temperature, exclude, with_entropy, last_slot_only)

    def sampled_softmax_loss(self, profile: Tuple[Tensor, Optional[Tensor], Tensor], pos: Tensor, samples: Tensor,
                             log_q: Tensor) -> Tensor:
        """Sampled softmax cross-entropy with the logQ correction: catalogue_softmax_loss with the
        catalogue replaced by K ids `samples` shared by every slot, drawn from a proposal Q with log_q [n_items] = log Q
        (sampling.ItemSampler).  Each valid slot's logsumexp runs over its positive and the samples that are not its
        positive (accidental hits removed; duplicates each count), every logit corrected by -log(K Q(i)).  Sample ids
        outside [1, n_items) contribute nothing.  With samples = arange(1, n_items) and uniform Q it equals
        catalogue_softmax_loss.  Same decoders, embeddings, dropout and errors as catalogue_softmax_loss."""
        from .catalogue_xent import sampled_softmax_loss

        return sampled_softmax_loss(self, profile, pos, samples, log_q)

    def listed_softmax_loss(self, profile: Tuple[Tensor, Optional[Tensor], Tensor], pos: Tensor, negatives) -> Tensor:
        """Softmax cross-entropy against a different list of negatives per user: hard negatives
        mined with retrieve (sampling.HardNegativeMiner), logged impressions, any per-user candidate list.  negatives: a
        catalogue.NegativeLists of [B, N] built for this model's n_items -- one list per user, shared by the user's L
        slots -- or a raw integer tensor [B, N], which builds one for this call and so costs a host sync per call.  Each
        valid slot's logsumexp runs over its positive and the entries of its user's list that are items and not its
        positive (duplicates each count), an entry's logit plus negatives.bias where one was given; ids outside
        [1, n_items) are padding, a slot whose list has no such entry pays 0.  With every list arange(1, n_items) it
        equals catalogue_softmax_loss.  No float atomics: the same call gives the same bits.  Same decoders, embeddings,
        dropout and errors as catalogue_softmax_loss."""
        from .catalogue_xent import listed_softmax_loss

        return listed_softmax_loss(self, profile, pos, negatives)

    def sampled_bce_loss(self, profile: Tuple[Tensor, Optional[Tensor], Tensor], pos: Tensor, pos_ctx: Tensor,
                         samples: Tensor, t: float = 0.75) -> Tensor:
        """Binary cross-entropy against K negatives shared by every slot, gBCE (Petrov & Macdonald, gSASRec; DESIGN.md
        section 16): pos = o_x[:, :L], pos_ctx = o_c[:, :L], `samples` K ids drawn uniformly.  Each valid slot pays
        beta softplus(-z+) for its positive (embedded with pos_ctx) and softplus(z_k) for every sample that is an item and not
        its positive, the sample embedded with the SLOT's context as the reference's negatives are (data.py); scalar mean
        over the valid slots.  beta = 1 - t (1 - K / (n_items - 1)): t = 0 is plain BCE over K negatives, t = 1 fully
        calibrated; t outside [0, 1] raises ValueError.  Same decoders, embeddings, dropout and errors as
        catalogue_softmax_loss."""
        from .catalogue_xent import sampled_bce_loss

        return sampled_bce_loss(self, profile, pos, pos_ctx, samples, t)

    # ---- full-catalogue top-k and ranks (include/carca_hip.h: carca_recommend / carca_rank_items) -
    def recommend(self, profile: Tuple[Tensor, Optional[Tensor], Tensor], context: Optional[Tensor], k: int = 10,
                  exclude="profile", candidates=None, allow_composed: bool = False) -> Tuple[Tensor, Tensor]:
        """The k best items of the whole catalogue per user: (scores [B, k] float32, ids [B, k] int64), best first.

        Scores equal what forward(profile, [(ids, attrs, context broadcast)]) returns for those items (eval mode: the
        candidates do not interact, carca.py:339).  profile = (p_x, p_a, p_c) as for forward (p_a may be None with an
        attribute table registered); context [B, n_ctx] is the context every candidate carries (data.py:180-185).
        exclude: "profile" (the profile's items), None, or an int [B, E] tensor of ids (0 = no entry).  Ties go to the
        smaller id; fewer than k eligible items pad with id 0 and score 0.  Needs model.eval(); L <= 64, a (d, H) with
        fused kernels built and 1 <= k <= 128.  The item-side tables are built on the first call and cached per weight
        version (item_table / context_matrix / recommend_tables).

        candidates: None (the whole catalogue), or a set S of item ids shared by the batch -- a catalogue.CandidateSet
        built for this model's n_items, or a raw 1-D integer tensor / bool mask [n_items], which builds one for this call
        and so costs a host sync per call.  The result is then the k best items of S minus the excluded ones, in the same
        order and with the same padding; a returned item's score is bit-identical to the unrestricted call's for that
        (user, item), and time and scratch ([B, |S|]) follow |S|, not n_items.  An empty S returns all zeros.

        allow_composed=True widens the envelope to what forward takes at d <= 128: L up to 1024 and any encoder head
        count, the profile side then running long_profile's composed encoder (several times slower per user than the
        fused blocks); the dot decoders at every (d, H), a cross-attention decoder at its built (d, H) geometries (past
        64 slots the sweep stages a user's valid slots 64 at a time: DESIGN.md section 19).  Inside the fused envelope
        the keyword changes nothing."""
        self._check_eval_built("recommend")
        return catalogue.recommend("recommend", _lib.RecommendDesc, "carca_recommend",
                                   self._model_side("recommend", profile, context, allow_composed), profile, k, exclude,
                                   candidates)

    def retrieve(self, profile: Tuple[Tensor, Optional[Tensor], Tensor], context: Optional[Tensor], k: int = 1000,
                 exclude="profile", candidates=None, allow_composed: bool = False) -> Tuple[Tensor, Tensor]:
        """recommend in depth, the first stage in front of a re-ranker, a filter or recommend_from: the k best items per
        user for 1 <= k <= catalogue.RETRIEVE_KMAX = 4096, (scores [B, k] float32, ids [B, k] int64), best first
        (DESIGN.md section 26).

        Every argument and the whole contract are recommend's: the order is the raw logit descending with ties to the
        smaller id (the link is applied to the selected logits only), id 0 and the excluded ids are never returned, fewer
        than k eligible items pad with id 0 and score 0, `candidates` restricts the call to a set (an empty one gives all
        zeros; scratch [B, |S|]), allow_composed widens the envelope, and the errors are recommend's under this call's
        name.  retrieve(k)[:, :j] equals retrieve(j) bit for bit in both outputs for every j <= k, and retrieve(k)
        equals recommend(k) bit for bit for every k <= 128: scoring and exclusion are recommend's launches, so a
        returned pair's score has recommend's / score_items' bits.  The result is bit-reproducible and does not depend on
        how many parts the selection split a user's row into (ops.TUNE_RETRIEVE_PARTS).  ids can go unchanged to
        recommend_from / score_items / score_items_at as `items` (id 0 scores 0 there)."""
        self._check_eval_built("retrieve")
        return catalogue.retrieve("retrieve", _lib.RecommendDesc, "carca_retrieve",
                                  self._model_side("retrieve", profile, context, allow_composed), profile, k, exclude,
                                  candidates)

    def recommend_sampled(self, profile: Tuple[Tensor, Optional[Tensor], Tensor], context: Optional[Tensor], k: int = 10,
                          temperature: float = 1.0, seed: Optional[int] = None, user_keys: Optional[Tensor] = None,
                          exclude="profile", candidates=None,
                          allow_composed: bool = False) -> Tuple[Tensor, Tensor, Tensor]:
        """recommend with exploration and logged propensities: per user, k items drawn WITHOUT
        replacement from softmax(logit / temperature) over the eligible items -- a Plackett-Luce list, in draw order --
        as (scores [B, k] float32, ids [B, k] int64, log_probs [B, k] float32), 1 <= k <= catalogue.RETRIEVE_KMAX.

        Eligibility, exclude, candidates, allow_composed and the envelope are recommend's.  scores[u, j] is
        link(raw logit), bit for bit what score_items / recommend return for that pair.  log_probs[u, j] =
        logit / temperature - logsumexp over user u's eligible items: the item's first-draw log-probability, the
        pi(a | x) of an IPS or doubly-robust estimator; catalogue.plackett_luce_log_prob(log_probs) gives the conditional
        log-probabilities of the ordered list.  Rows with fewer than k eligible items pad with (0, 0, -inf).

        The draw is Gumbel top-k: the k largest of logit / temperature + g, g iid standard Gumbel hashed from (seed, the
        user's key, the item id) -- include/carca_hip.h states the hash.  seed: an int (mod 2^64), or None: one from
        torch's CPU generator (torch.manual_seed makes the sequence reproducible).  user_keys: None (row u's key is u) or
        an int [B] tensor, e.g. user or request ids.  So: the same arguments and seed give the same bits;
        recommend_sampled(k)[:, :j] equals recommend_sampled(j); a row depends on (seed, its key, its profile, context
        and exclusion) only, not on the batch around it; under candidates=S the result is the unrestricted perturbed
        order with the items outside S struck out.  temperature must be a finite float > 0 and a normal fp32 number (>= 1.18e-38); as
        it falls the list approaches recommend's.  The noise has 23 bits: an item more than 19.4 in logit / temperature below the user's
        best is never drawn ahead of it.  Scratch: a second [B, n_items] fp32 buffer beside recommend's."""
        self._check_eval_built("recommend_sampled")
        return catalogue.recommend_sampled("recommend_sampled", _lib.RecommendDesc, "carca_recommend_sampled",
                                           self._model_side("recommend_sampled", profile, context, allow_composed),
                                           profile, k, temperature, seed, user_keys, exclude, candidates)

    def log_prob_items(self, profile: Tuple[Tensor, Optional[Tensor], Tensor], context: Optional[Tensor], items: Tensor,
                       temperature: float = 1.0, exclude="profile", candidates=None,
                       allow_composed: bool = False) -> Tuple[Tensor, Tensor, Tensor]:
        """log pi(item | user) of listed items under recommend_sampled's policy: the numerator of
        an IPS / SNIPS estimator whose denominator recommend_sampled logged.  -> (log_probs [B, N] float32, lse [B]
        float32, entropy [B] float32).

        items: an int [B, N] tensor, a list per user -- any length (N = 0 too), any order, duplicates allowed.
        Eligibility, exclude, candidates, allow_composed, the envelope and the temperature check are recommend_sampled's.
        With z = logit / temperature: lse[u] is the logsumexp of z over user u's eligible items (-inf when there is none);
        log_probs[u, j] = z - lse[u] where items[u, j] is eligible and exactly -inf otherwise (id 0, an excluded id, an id
        outside candidates, a negative id, an id >= n_items -- 2^40 does not wrap into range); entropy[u] =
        -sum p log p over the eligible items in nats (0 when there is none), so exp(entropy) is the effective number of
        items the policy chooses among -- how exploratory a temperature is, before it ships.

        For the ids recommend_sampled(temperature=t, exclude=e, candidates=S) returned, log_prob_items(items=ids,
        temperature=t, exclude=e, candidates=S)[0] equals that call's log_probs bit for bit (padding gives -inf on both
        sides); under another checkpoint or temperature it is the target policy's side of the ratio
        (catalogue.policy_log_ratio, off_policy_estimate; train.off_policy_value runs a whole log).  A user's row, lse and
        entropy do not depend on the batch around it, on the order of the list or on any launch shape.  Scratch:
        recommend's buffer plus 12 bytes per user and 1024 items -- no second buffer."""
        self._check_eval_built("log_prob_items")
        return catalogue.log_prob_items("log_prob_items", _lib.RecommendDesc, "carca_log_prob_items",
                                        self._model_side("log_prob_items", profile, context, allow_composed),
                                        profile, items, temperature, exclude, candidates)

    def rank_items(self, profile: Tuple[Tensor, Optional[Tensor], Tensor], context: Optional[Tensor], items: Tensor,
                   exclude="profile", candidates=None, allow_composed: bool = False) -> Tuple[Tensor, Tensor]:
        """Exact full-catalogue ranks of listed items: (scores [B, N] float32, ranks [B, N] int64).

        items: an int32 / int64 [B, N] tensor, 1 <= N <= 128.  ranks[u, j] is the 0-based number of ELIGIBLE catalogue
        items (id != 0, not excluded) that come before items[u, j] in recommend's order (logit descending, ties to the
        smaller id) -- the position recommend would give it, at any depth; an excluded item still gets the position it
        would take.  scores[u, j] is what forward / recommend returns for it.  An id of 0 or outside [0, n_items) gives
        rank -1 and score 0 (no host check, no out-of-bounds read).  profile, context, exclude and the envelope are
        recommend's; the item-side tables come from the same caches.

        candidates: as recommend's.  With a set S, ranks[u, j] counts the eligible items OF S (in S, not excluded) that
        come before items[u, j] -- the position recommend(candidates=S) would give it; a target outside S, like an
        excluded or repeated one, still gets the position it would take, and with an empty S every valid target has
        rank 0.  scores keep their meaning and their bits.

        allow_composed: as recommend's."""
        self._check_eval_built("rank_items")
        return catalogue.rank_items("rank_items", _lib.RankDesc, "carca_rank_items",
                                    self._model_side("rank_items", profile, context, allow_composed), profile, items,
                                    exclude, candidates)

    # ---- a candidate list per user (include/carca_hip.h: carca_score_lists / carca_recommend_lists) ----
    def score_items(self, profile: Tuple[Tensor, Optional[Tensor], Tensor], context: Optional[Tensor], items: Tensor,
                    allow_composed: bool = False) -> Tensor:
        """The scores of each user's own list of items, from the per-item tables: [B, N] float32.

        items: an int32 / int64 [B, N] tensor, N >= 1 and as long as the caller likes (B * N must fit an int): row u is
        user u's list, e.g. a retriever's candidates.  scores[u, j] is what forward / recommend / rank_items returns
        for (u, items[u, j]), bit for bit rank_items' and recommend's score of that pair.  An id of 0 or outside
        [1, n_items) scores 0 (no host check, no out-of-bounds read); duplicates are each scored, caller order is
        kept, nothing is excluded.  One launch with the user staged once per workgroup, no scratch, no host sync.
        profile, context and the envelope are recommend's; allow_composed: as recommend's."""
        self._check_eval_built("score_items")
        return catalogue.score_items("score_items", self._model_side("score_items", profile, context, allow_composed),
                                     profile, items)

    def recommend_from(self, profile: Tuple[Tensor, Optional[Tensor], Tensor], context: Optional[Tensor], items: Tensor,
                       k: int = 10, exclude="profile", allow_composed: bool = False) -> Tuple[Tensor, Tensor]:
        """The k best items of each user's OWN list: (scores [B, k] float32, ids [B, k] int64), best first.

        items: as score_items' -- an int [B, N] tensor of any length N, a different list per user.  Per user the
        eligible items are the distinct ids of its row that are items (in [1, n_items)) minus the excluded ones;
        order and padding are recommend's: score descending, ties to the smaller id, fewer than k eligible items pad
        with id 0 and score 0.  Row u is bit for bit row 0 of recommend((p_x[u:u+1], p_a[u:u+1], p_c[u:u+1]),
        context[u:u+1], k, exclude_u, candidates=the distinct valid ids of items[u]), in both outputs, without a
        CandidateSet and without a host sync.  Up to catalogue.LIST_FUSED_MAX = 1024 entries the call is one launch
        with one workgroup per user; a longer list is sorted per row on the device, scored into stream scratch [B, N]
        and selected per row -- the same result either way.  exclude: recommend's three forms; 1 <= k <= 128.
        profile, context and the envelope are recommend's; allow_composed: as recommend's."""
        self._check_eval_built("recommend_from")
        return catalogue.recommend_from("recommend_from",
                                        self._model_side("recommend_from", profile, context, allow_composed), profile,
                                        items, k, exclude)

    # ---- several request contexts per user (include/carca_hip.h: CarcaContexts) -------------------------
    def score_items_at(self, profile: Tuple[Tensor, Optional[Tensor], Tensor], contexts: Tensor, items: Tensor,
                       allow_composed: bool = False) -> Tensor:
        """score_items under C request contexts per user in one call: [B, C, N] float32.

        contexts: a float [B, C, n_ctx] tensor, C >= 1 -- "tonight, tomorrow morning, at the weekend"; C is not capped.
        Slice [:, c] is score_items(profile, contexts[:, c], items), bit for bit.  The profile side (embedding, encoder
        blocks, final norm, K, V -> u) runs once, each (head, slot, item) dot product is computed once, and a further
        context costs its own three small row products and a bias, two exp2 and two FMAs per (slot, head) (DESIGN.md
        section 25).  items, the treatment of ids that are no items and allow_composed are score_items'.  The envelope
        is recommend's with two differences: an embedding without a context matrix (AttrEmbedding, IdEmbedding,
        MLPIdEmbedding: the score does not depend on the candidate's context) raises -- call score_items -- and so does
        a cross-attention decoder over a profile of more than 64 slots -- call score_items per context."""
        self._check_eval_built("score_items_at")
        side = self._model_side_at("score_items_at", "score_items", profile, contexts, allow_composed)
        return catalogue.score_items_at("score_items_at", side, profile, contexts, items)

    def best_context(self, profile: Tuple[Tensor, Optional[Tensor], Tensor], contexts: Tensor, items: Tensor,
                     allow_composed: bool = False) -> Tuple[Tensor, Tensor]:
        """At which of a user's C contexts each listed item scores best: (scores [B, N] float32, which [B, N] int64).

        Per (user, list entry) the largest LOGIT over the C contexts of score_items_at; a tie goes to the smaller context
        index.  scores is that logit through the model's link, with score_items_at's bits (= its maximum over dim 1);
        which is its context index.  An id that is no item gives score 0 and index -1.  One launch; no [B, C, N] buffer
        is formed.  Arguments and envelope: score_items_at's."""
        self._check_eval_built("best_context")
        side = self._model_side_at("best_context", "score_items", profile, contexts, allow_composed)
        return catalogue.best_context("best_context", side, profile, contexts, items)

    def recommend_at(self, profile: Tuple[Tensor, Optional[Tensor], Tensor], contexts: Tensor, k: int = 10,
                     exclude="profile", candidates=None, allow_composed: bool = False,
                     max_scratch_bytes: int = 1 << 30) -> Tuple[Tensor, Tensor]:
        """recommend under C request contexts per user in one call: (scores [B, C, k] float32, ids [B, C, k] int64).

        contexts: as score_items_at's.  Slices [:, c] of both outputs are recommend(profile, contexts[:, c], k, exclude,
        candidates), bit for bit: order, ties to the smaller id, padding with id 0 and score 0; user u's exclusion
        applies to all its contexts.  The profile side runs once and the catalogue is swept once, the head dot products
        shared by the contexts; exclusion and selection then run per (user, context).  The raw logits are
        [users, C, n_slots] floats of stream scratch (n_slots = n_items, or the candidate count): the users go in chunks
        that keep it within max_scratch_bytes, with no host sync, and the result does not depend on the chunking; a
        budget that does not hold one user's [C, n_slots] raises.  k, exclude, candidates and allow_composed are
        recommend's; the envelope is score_items_at's."""
        self._check_eval_built("recommend_at")
        side = self._model_side_at("recommend_at", "recommend", profile, contexts, allow_composed)
        return catalogue.recommend_at("recommend_at", side, profile, contexts, k, exclude, candidates, max_scratch_bytes)

    # ---- item groups (include/carca_hip.h: carca_recommend_groups / carca_recommend_capped) -------------
    def _catalogue_size(self) -> Optional[int]:
        """n_items where no launch is needed to know it: the id table's rows, else the registered attribute table's."""
        emb = self.embeds
        if isinstance(getattr(emb, "items_embed", None), nn.Embedding):
            return emb.items_embed.num_embeddings
        table = emb.attr_table() if hasattr(emb, "attr_table") else None
        return None if table is None else table.shape[0]

    def recommend_by_group(self, profile: Tuple[Tensor, Optional[Tensor], Tensor], context: Optional[Tensor], groups,
                           k: int = 10, exclude="profile", allow_composed: bool = False) -> Tuple[Tensor, Tensor]:
        """The k best items of EVERY group per user, in one call: (scores [B, G, k] float32, ids [B, G, k] int64).

        groups: a catalogue.ItemGroups built for this model's n_items (a group label per item; an item without a label
        is never returned).  Row (u, g) is bit for bit row u of recommend(profile, context, k, exclude,
        candidates=groups.members(g), allow_composed), in both outputs: logit descending, ties to the smaller id,
        excluded ids never, padded with id 0 and score 0 where the group has fewer than k eligible items; an empty group
        is all padding.  The profile side runs once and the catalogue is swept once, in group-major order; one selection
        launch picks every (user, group) list.  No host sync.  There is no candidates= argument: restrict the call by
        leaving items ungrouped.  profile, context, exclude, 1 <= k <= 128, the envelope and allow_composed are
        recommend's."""
        self._check_eval_built("recommend_by_group")
        side = self._model_side("recommend_by_group", profile, context, allow_composed)
        return catalogue.recommend_by_group("recommend_by_group", side, profile, groups, k, exclude, self._catalogue_size())

    def recommend_capped(self, profile: Tuple[Tensor, Optional[Tensor], Tensor], context: Optional[Tensor], groups,
                         k: int = 10, max_per_group: int = 1, exclude="profile",
                         allow_composed: bool = False) -> Tuple[Tensor, Tensor]:
        """The k best items per user with at most max_per_group from any one group ("at most two per brand"):
        (scores [B, k] float32, ids [B, k] int64).

        The result is recommend's order over the grouped, non-excluded items walked from the best, skipping an item once
        its group has max_per_group items in the list, until k are taken; ties go to the smaller id, across groups too;
        padding as recommend's; items without a label are not eligible.  max_per_group >= k leaves the cap inactive: the
        call is then recommend over the grouped items.  A returned item's score has recommend's bits.  The device side
        takes every group's best min(k, max_per_group) and then the k best of their union, through a
        [B, G, min(k, max_per_group)] buffer of 64-bit keys; a buffer beyond 1 GiB raises CarcaHipError (split the batch).
        No host sync.  groups, profile, context, exclude, k, the envelope and allow_composed: as recommend_by_group."""
        self._check_eval_built("recommend_capped")
        side = self._model_side("recommend_capped", profile, context, allow_composed)
        return catalogue.recommend_capped("recommend_capped", side, profile, groups, k, max_per_group, exclude,
                                          self._catalogue_size())

    # ---- the k best users per listed item (include/carca_hip.h: carca_recommend_users) ------------------
    def recommend_users(self, profile: Tuple[Tensor, Optional[Tensor], Tensor], context: Optional[Tensor], items,
                        k: int = 10, exclude="profile", user_ids: Optional[Tensor] = None,
                        allow_composed: bool = False) -> Tuple[Tensor, Tensor, Tensor]:
        """The k best USERS of the batch for each listed item ("who should hear about these Q items"):
        (scores [Q, k] float32, users [Q, k] int64, item_ids [Q] int64).

        items: a catalogue.CandidateSet built for this model's n_items, or a raw 1-D integer tensor / bool mask
        [n_items], which builds one for this call and so costs a host sync, as recommend(candidates=) does.  Rows follow
        the set's ascending distinct ids, returned as item_ids; an empty set returns empty outputs.  Row q holds the k
        eligible users with the largest LOGIT for item item_ids[q], best first, ties to the smaller user id;
        scores[q, j] is bit for bit score_items' / recommend's score of that (user, item) pair; fewer than k eligible
        users pad with user -1 and score 0.  User u is not eligible for item i where `exclude` lists i for u (recommend's
        three forms; "profile" reads as "has it already"), nor where user_ids[u] is negative (a row dropped without
        reshaping the batch).  user_ids: an int32 / int64 [B] tensor of ids below 2^31 naming the rows, None = the row
        index.  The result does not depend on scheduling, and a larger audience over many batches comes from
        catalogue.AudienceTopK (train.audience walks a loader), whose result does not depend on the batching either.
        1 <= k <= 128; eval mode; profile, context, the envelope and allow_composed are recommend's."""
        self._check_eval_built("recommend_users")
        return catalogue.recommend_users(self, profile, context, items, k, exclude, user_ids, allow_composed)

    # ---- which profile slots drive a score (include/carca_hip.h: carca_explain_lists) ------------------
    def _check_explainable(self, what: str) -> None:
        self._check_eval_built(what)
        if not isinstance(self.decoder, CrossAttentionBlock):
            raise CarcaHipError(f"{what}: decoder {type(self.decoder).__name__} has no attention over the profile to "
                                "decompose: its eval score reads the last profile slot only (a cross-attention decoder "
                                "is needed)")

    def explain_items(self, profile: Tuple[Tensor, Optional[Tensor], Tensor], context: Optional[Tensor], items: Tensor,
                      allow_composed: bool = False) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
        """Why each item of each user's own list scores what it scores: (scores [B, N], base [B, N],
        contrib [B, N, L], weights [B, H, N, L]), all float32.

        In eval mode the cross-attention decoder's logit is additive over the profile slots:
        logit(u, i) = base(u, i) + sum_t contrib[u, i, t], with contrib[u, j, t] = sum_h weights[u, h, j, t] * U[u, t, h],
        U the decoder FFN folded into the value rows (w_ffn,h . V[u, t, h]) and base the FFN bias plus, with the
        residual, w_ffn . e(i, context).  scores is score_items' output for the same arguments, bit for bit, and
        sigmoid(base + contrib.sum(-1)) reproduces it up to fp32 rounding: a true decomposition, not a heuristic.
        weights[u, h, j, t] is the reference's attention weight (MultiHeadAttention.forward(..., return_w=True)) of head
        h, query items[u, j], key slot t.  Weights and contributions are exactly 0 at a padding slot (p_x[u, t] == 0,
        interior zeros included), for an id that is no item (0, or outside [1, n_items): score and base 0 too) and for
        an empty profile.  items, profile, context, the envelope and allow_composed are score_items'; one launch, no
        host sync.  A dot decoder raises CarcaHipError."""
        self._check_explainable("explain_items")
        return catalogue.explain_items("explain_items", self._model_side("explain_items", profile, context, allow_composed),
                                       profile, items)

    def explain_top_slots(self, profile: Tuple[Tensor, Optional[Tensor], Tensor], context: Optional[Tensor],
                          items: Tensor, m: int = 3, allow_composed: bool = False
                          ) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
        """The m profile slots that contribute most to each (user, item) score: (scores [B, N], base [B, N],
        slots [B, N, m] int64, slot_items [B, N, m] int64, contrib [B, N, m] float32).

        Per (u, j) the m valid slots with the largest explain_items contribution, in descending order, ties to the later
        slot (the more recent interaction); slots are positions in [0, L), slot_items the profile ids p_x there, contrib
        bit for bit the matching entries of explain_items' contrib.  Fewer than m valid slots, and an id that is no
        item, pad with slot -1, item 0 and contribution 0.  1 <= m <= catalogue.EXPLAIN_TOP_MAX = 8.  No [B, N, L]
        buffer exists on this path.  Everything else is explain_items'."""
        self._check_explainable("explain_top_slots")
        side = self._model_side("explain_top_slots", profile, context, allow_composed)
        return catalogue.explain_top_slots("explain_top_slots", side, profile, items, m)

    def recommend_explained(self, profile: Tuple[Tensor, Optional[Tensor], Tensor], context: Optional[Tensor],
                            k: int = 10, m: int = 3, exclude="profile", candidates=None, allow_composed: bool = False
                            ) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
        """recommend with its reasons ("because you bought X and Y"): (scores [B, k], ids [B, k],
        slot_items [B, k, m] int64, contrib [B, k, m] float32).

        scores and ids are recommend's for the same arguments, bit for bit; the last two are explain_top_slots over
        those ids (the padding id 0 explains as an id that is no item: items 0, contributions 0).  The profile side
        runs once for both launches.  k, exclude, candidates and allow_composed are recommend's, m explain_top_slots'."""
        self._check_explainable("recommend_explained")
        side = self._model_side("recommend_explained", profile, context, allow_composed)
        return catalogue.recommend_explained("recommend_explained", side, profile, k, m, exclude, candidates)

    # ---- item-to-item top-k (include/carca_hip.h: carca_similar_items) ---------------------------------
    def similar_items(self, items: Optional[Tensor] = None, k: int = 10, metric: str = "cosine", exclude_self: bool = True,
                      candidates=None, max_scratch_bytes: int = 1 << 30) -> Tuple[Tensor, Tensor]:
        """The k items closest to each listed item in the space of the item table T[i] = e(i, 0) -- the row every
        catalogue call scores an item by: (scores [Q, k] float32, ids [Q, k] int64), best first, on the device.

        items: an int [Q] tensor of item ids (duplicates allowed), or None for every item (outputs [n_items, k], row i
        for item i, row 0 padding).  metric "cosine": ((T[q] . T[i]) * r_q) * r_i with r = 1 / max(||T[.]||, 1e-12) in
        fp32 (an all-zero row scores 0); "dot": T[q] . T[i]; anything else raises ValueError.  Eligible neighbours are
        ids 1 .. n_items - 1, minus the query itself when exclude_self (items whose rows duplicate it stay), intersected
        with `candidates` when given (a catalogue.CandidateSet, or a raw tensor / mask that builds one for this call and
        costs a host sync; the query need not be in it).  Order and padding are recommend's: score descending, ties to
        the smaller id, fewer than k eligible items pad with id 0 and score 0; a query id outside [1, n_items) gives a
        fully padded row; scores are the raw metric.  1 <= k <= 128.  Bit-reproducible, and a pair's score bits do not
        depend on the query's position, on the candidates or on max_scratch_bytes: the queries go in chunks whose
        [Qc, C] score buffer stays within it (C = n_items or |S|; one 64-query block at least), with no sync between
        them.  Runs under no_grad in train and eval mode alike; embeddings that read attributes need
        register_attr_table.  T and r are cached per weight version."""
        catalogue.similar_args("similar_items", items, k, metric)
        with torch.no_grad():
            emb = self.embeds
            T = emb.item_table()
            return catalogue.similar_items("similar_items", T, emb.d, partial(_item_rnorm, emb, T), items, k, metric,
                                           exclude_self, candidates, max_scratch_bytes)

    # ---- diversity re-ranking (include/carca_hip.h: carca_mmr_rerank) ----------------------------------
    def recommend_diverse(self, profile: Tuple[Tensor, Optional[Tensor], Tensor], context: Optional[Tensor], k: int = 10,
                          pool: int = 128, lam: float = 0.7, metric: str = "cosine", exclude="profile", candidates=None,
                          allow_composed: bool = False, normalize: bool = True) -> Tuple[Tensor, Tensor, Tensor]:
        """recommend's `pool` best items per user, re-ranked for diversity by maximal marginal relevance in the space of
        the item table T[i] = e(i, 0): (scores [B, k] float32, ids [B, k] int64 in selection order, ild [B] float32).

        The pool is self.recommend(profile, context, k=pool, exclude, candidates, allow_composed), unchanged; then, k
        times, the untaken pool item with the largest lam * rel - (1 - lam) * max_{s taken} sim(i, s) is taken (ties to
        the better pool position: better score, then smaller id).  rel is the pool score normalised to [0, 1] per user
        (normalize=True) or the score itself; sim is similar_items' "cosine" or "dot" over T, with the cached reciprocal
        norms.  scores are recommend's for the taken items; ild is the list's intra-list diversity, the mean of 1 - sim
        over its pairs (0 with fewer than two items); fewer than k eligible items pad with id 0 and score 0.  lam = 1 is
        recommend(k) bit for bit; lam = 0 is pure diversity after the best item.  Errors and envelope are recommend's,
        plus 1 <= k <= pool <= 128 (CarcaHipError) and lam in [0, 1], metric "cosine" / "dot" (ValueError)."""
        catalogue.mmr_args("recommend_diverse", k, pool, lam, metric)
        s, i = self.recommend(profile, context, k=pool, exclude=exclude, candidates=candidates, allow_composed=allow_composed)
        with torch.no_grad():
            emb = self.embeds
            T = emb.item_table()
            return catalogue.mmr_rerank("recommend_diverse", s, i, T, emb.d, k, lam, metric, normalize,
                                        partial(_item_rnorm, emb, T))

    # ---- inference: one host call per forward (include/carca_hip.h: carca_forward) -----------------------------
    def _fused_ok(self, trace) -> bool:
        if trace is not None or len(self.encoder) > _lib.MAX_BLOCKS or not self._fusable():
            return False
        if self.training and (self.dropout.p > 0 or self.decoder.drop_p() > 0 or
                              any(b.drop_p() > 0 for b in self.encoder)):
            return False
        return True

    def _forward_fused(self, profile, targets, events=None, train: Optional[dict] = None) -> List[Tensor]:
        """One host call for the whole forward (carca_forward).  train: None = inference (workspaces cached per shape);
        a dict = the TRAINING forward: fresh buffers, the backward's saved tensors and the dropout sites, all handed back
        through that dict (the keys autograd._CarcaFn keeps in its state)."""
        import ctypes as C

        p_x, p_a, p_c = profile
        emb, dec = self.embeds, self.decoder
        d, H = emb.d, dec.attn.H
        dev = p_x.device
        ops._need_cuda(p_x)
        dpi, _, _ = ops.padded_dims(d, H)
        B, L = p_x.shape
        g = emb.feats_embed.out_features
        table = emb.attr_table()
        n_ctx = p_c.shape[-1]
        n_attrs = table.shape[1] if table is not None else p_a.shape[-1]
        Ns = tuple(int(t[0].shape[1]) for t in targets)
        key = (str(dev), B, L, Ns, n_attrs, n_ctx, table is not None)
        rows = B * (L + sum(Ns))
        f32 = dict(dtype=torch.float32, device=dev)
        if train is None:
            plan = self.__dict__.get("_plan")
            if plan is None or plan["key"] != key:
                plan = dict(key=key, D=_lib.ForwardDesc(), zq=torch.empty(rows, d + g, **f32),
                            es=[torch.empty(B, T, dpi, **f32) for T in (L,) + Ns],
                            xw=[torch.empty(B, L, dpi, **f32) for _ in range(2)])
                self.__dict__["_plan"] = plan
        else:  # everything the backward reads must outlive this call: fresh buffers
            plan = dict(D=_lib.ForwardDesc(), zq=torch.empty(rows, d + g, **f32),
                        es=[torch.empty(B, T, dpi, **f32) for T in (L,) + Ns], xw=[None, None])
        D = plan["D"]
        segs = [(p_x, p_a, p_c)] + [tuple(t) for t in targets]
        keep = []
        pos = emb._pos(L)
        for i, (x, a, c) in enumerate(segs):
            ops._need_cuda(x, a, c)
            T = x.shape[1]
            if x.shape[0] != B or c.shape != (B, T, n_ctx) or (a is not None and a.shape != (B, T, n_attrs)):
                raise CarcaHipError("forward: ids / attrs / ctx shapes do not match")
            if a is None and table is None:
                raise CarcaHipError("forward: attrs is None and no attribute table is registered")
            x32 = ops._ids32(x)
            S = D.segs[i]
            S.ids, S.e_out, S.rows, S.T = x32.data_ptr(), plan["es"][i].data_ptr(), B * T, T
            S.add_pos = int(i == 0 and pos is not None)
            if a is not None:
                a, a_bs = ops._btk_view(a)
                S.attrs, S.attrs_bstride, S.attrs_table = a.data_ptr(), a_bs, None
            else:
                S.attrs, S.attrs_bstride, S.attrs_table = None, 0, table.data_ptr()
                S.attrs_table_rows = table.shape[0]
            if n_ctx > 0:
                c, c_bs = ops._btk_view(c)
                S.ctx, S.ctx_bstride = c.data_ptr(), c_bs
            keep += [x32, a, c]
        D.ngroups, D.B, D.L, D.d, D.g, D.H = len(targets), B, L, d, g, H
        D.n_attrs, D.n_ctx, D.n_blocks, D.ld_e = n_attrs, n_ctx, len(self.encoder), dpi
        prm = [emb.items_embed.weight, emb.feats_embed.weight, emb.feats_embed.bias, emb.joint_embed.weight,
               emb.joint_embed.bias]
        for t in prm:
            ops._need_cuda(t)
        D.items_w, D.feats_w, D.feats_b, D.joint_w, D.joint_b = [t.data_ptr() for t in prm]
        emb.bind_split_weights(n_attrs)
        if pos is not None:
            pos = pos.detach().contiguous()
            keep.append(pos)
        D.pos = pos.data_ptr() if pos is not None else None
        D.zq = plan["zq"].data_ptr()
        if self.__dict__.get("_fold") and not self.training:
            wc, bias_c = emb.folded_weights()
            keep += [wc, bias_c]
            D.fold_wc, D.fold_bias, D.fold_ldwc = wc.data_ptr(), bias_c.data_ptr(), wc.stride(0)
        else:
            D.fold_wc, D.fold_bias, D.fold_ldwc = None, None, 0
        D.z_table, D.ld_z_table = None, 0
        if train is None and not self.training and D.fold_wc is None and USE_Z_TABLE:
            zt = emb.z_table()  # (inference: the item term of the joint embedding per item, cached per weight version)
            keep.append(zt)
            D.z_table, D.ld_z_table = zt.data_ptr(), zt.stride(0)
        if train is None:
            D.x_work[0], D.x_work[1] = plan["xw"][0].data_ptr(), plan["xw"][1].data_ptr()
        repack: list = []  # (after a training step every module repacks: one launch for all of them)
        for i, blk in enumerate(self.encoder):
            blk._check_mode()
            D.sa[i] = blk.weights_struct(dev, repack)
            keep.append(blk.__dict__["_pack_cache"])
            D.sa_residual[i] = int(bool(blk.residual))
        D.ca = dec.weights_struct(dev, self.norm, repack)
        ops.pack_many(repack)
        D.ca_residual, D.training = int(bool(dec.residual)), int(bool(self.training))
        # the groups' scores are written as column blocks of ONE [B, sum N] tensor: what carca.py:431's torch.cat builds,
        # without the copy (and without the split / re-gather of its gradient in the backward pass)
        ys = JointScores()
        ys.joint = torch.empty(B, sum(Ns), dtype=torch.float32, device=dev)
        off = 0
        for gi, N in enumerate(Ns):
            y = ys.joint[:, off: off + N]
            ys.append(y)
            D.y[gi], D.N[gi] = y.data_ptr(), N
            off += N
        D.ldy = sum(Ns)
        D.p_normed = None
        if train is not None:
            _, _, dpo = ops.padded_dims(d, H)
            u8 = lambda *sh: torch.empty(*sh, dtype=torch.uint8, device=dev)  # noqa: E731
            mk = lambda n, w_: torch.empty(n, w_, **f32)  # noqa: E731
            seed = ops.new_dropout_seed() if self.training else 0
            p_emb = float(self.dropout.p) if self.training else 0.0
            p_blk = max([b.drop_p() for b in self.encoder], default=0.0)
            if any(b.drop_p() != p_blk for b in self.encoder):
                raise CarcaHipError("forward: the blocks' dropout probabilities differ (one value per call)")
            p_ca = dec.drop_p()
            blocks, x_prev = [], plan["es"][0]
            for i, blk in enumerate(self.encoder):
                y_i = torch.empty(B, L, dpi, **f32)
                D.x_out[i] = y_i.data_ptr()
                sv = dict(qn=mk(B * L, dpi), qh=mk(B * L, dpo), kh=mk(B * L, dpo), vh=mk(B * L, dpo), r=mk(B * L, dpi),
                          s2=mk(B * L, dpi), h1=mk(B * L, dpi))
                if p_blk > 0:
                    sv.update(m_attn=u8(B, blk.attn.H, L, L), m_ffn1=u8(B * L, dpi), m_ffn2=u8(B * L, dpi))
                S = D.sa_save[i]
                for k in ("qn", "qh", "kh", "vh", "r", "s2", "h1", "m_attn", "m_ffn1", "m_ffn2"):
                    setattr(S, k, sv[k].data_ptr() if k in sv else None)
                sv["x_in"], sv["p"] = x_prev, p_blk
                blocks.append(sv)
                x_prev = y_i
            p_normed = torch.empty(B, L, dpi, **f32)
            D.p_normed = p_normed.data_ptr()
            csave = dict(kh=mk(B * L, dpo), vh=mk(B * L, dpo), qh=[mk(B * N, dpo) for N in Ns], p=p_ca)
            D.ca_save.kh, D.ca_save.vh = csave["kh"].data_ptr(), csave["vh"].data_ptr()
            if p_ca > 0:
                csave["m_attn"] = [u8(B, H, N, L) for N in Ns]
            for gi in range(_lib.MAX_GROUPS):
                D.ca_save.qh[gi] = csave["qh"][gi].data_ptr() if gi < len(Ns) else None
                D.ca_save.m_attn[gi] = csave["m_attn"][gi].data_ptr() if (p_ca > 0 and gi < len(Ns)) else None
            m_embed = u8(B * L, d) if p_emb > 0 else None
            D.save_blocks = D.save_cross = 1
            D.p_embed, D.p_block, D.p_cross, D.seed = p_emb, p_blk, p_ca, seed
            D.seed_offset = ops.dropout_seed_offset_ptr()
            D.m_embed = m_embed.data_ptr() if m_embed is not None else None
            train.update(es=plan["es"], zq=plan["zq"], blocks=blocks, enc_out=x_prev, p_normed=p_normed, csave=csave,
                         cw=D.ca, m_embed=m_embed, p_emb=p_emb, keep=(keep, D))
        ev = (C.c_void_p * len(events))(*events) if events is not None else None
        D.n_events = len(events) if events is not None else 0
        lib = _lib.load()
        if train is None and not self.training and D.fold_wc is None and isinstance(emb, AllEmbedding):
            # (evaluation: P rows of items an earlier batch multiplied come from the module's per-item cache)
            # (dense as soon as one segment brings its attribute rows: their bytes are then compared, gathered rows included)
            fc = emb.feat_cache(n_attrs, table if all(sg[1] is None for sg in segs) else None)
            if fc is not None:
                _lib.check(lib.carca_feat_cache_arm(C.byref(fc)), "feat_cache_arm")
        _lib.check(lib.carca_forward(C.byref(D), ev, ops._stream()), "forward")
        return ys

    def forward_nograd(self, profile, targets, trace: Optional[dict] = None) -> List[Tensor]:
        p_x, p_a, p_c = profile
        if self._composed(profile, targets):
            from . import long_profile

            return long_profile.forward(self, profile, targets, trace)
        if self._fused_ok(trace):
            return self._forward_fused(profile, targets, events=ops.fused_events())
        d = self.embeds.d
        H = self._heads()
        dpi, _, _ = ops.padded_dims(d, H)
        segs = [(p_x, p_a, p_c, False)] + [(o_x, o_a, o_c, True) for (o_x, o_a, o_c) in targets]
        es, _ = self.embeds.embed_segments(segs, ld_e=dpi)
        x = es[0]
        seed = ops.new_dropout_seed() if self.training else 0
        if self.training and self.dropout.p > 0:  # carca.py:416
            ops.dropout_fwd(x, d, float(self.dropout.p), seed, 1000)
        if trace is not None:
            trace["p_embed"] = x[..., :d]
            for gi in range(len(targets)):
                trace[f"o_embed{gi}"] = es[gi + 1][..., :d]
        for i, blk in enumerate(self.encoder):
            blk._check_mode()
            bp = blk.drop_p()
            x = ops.sa_block_fwd(x, p_x, blk.weights_struct(x.device), d, blk.attn.H, blk.residual,
                                 drop=(bp, seed, 4 * i) if bp > 0 else None)
            if trace is not None:
                trace[f"block{i}"] = x[..., :d]
        if not isinstance(self.decoder, CrossAttentionBlock):
            # dot decoders: stand-alone final LayerNorm (carca.py:421), then a row dot per target (carca.py:352-399)
            B, L = p_x.shape
            p_n = ops.layernorm_fwd(x.view(B * L, -1), self.norm.weight, self.norm.bias, d, dpi)
            if trace is not None:
                trace["p_final"] = p_n.view(B, L, dpi)[..., :d]
            ys, _ = self.decoder.score_groups(p_n, [e.view(-1, dpi) for e in es[1:]], [e.shape[1] for e in es[1:]], B, L,
                                              d, dpi)
            return ys
        self.decoder._check_mode()
        H = self.decoder.attn.H
        groups = [(es[gi + 1], targets[gi][0]) for gi in range(len(targets))]
        dp = self.decoder.drop_p()
        if dp > 0:
            ys, p_normed, _ = ops.cross_score_fwd(x, p_x, groups, self.decoder.weights_struct(x.device, self.norm), d, H,
                                                  self.decoder.residual, self.training, save=True,
                                                  drop=(dp, seed, 2000))
        else:
            ys, p_normed = ops.cross_score_fwd(x, p_x, groups, self.decoder.weights_struct(x.device, self.norm), d, H,
                                               self.decoder.residual, self.training, want_normed=trace is not None)
        if trace is not None:
            trace["p_final"] = p_normed[..., :d]
        return ys


# ------------------------------------------------------------------------------------------------
# KNN baseline (knn.py:8-21)
# ------------------------------------------------------------------------------------------------


class KNN(Model):
    """The reference's attribute-similarity baseline: score = attrs(last profile item) . attrs(target), no parameters.
    Extension: register_attr_table(attrs) lets profile/target attribute tensors be None (rows gathered by id on the
    device), as for AllEmbedding; with it registered, recommend / rank_items rank the whole catalogue (its rows) as
    CARCA's methods do."""

    def __init__(self):
        super().__init__()
        self._attr_table: Optional[Tensor] = None

    def register_attr_table(self, attrs: Optional[Tensor]) -> None:
        self._attr_table = None if attrs is None else attrs.detach().to(torch.float32).contiguous()
        self.__dict__.pop("_i8_cache", None)
        self.__dict__.pop("_similar_cache", None)

    def __getstate__(self):
        state = dict(super().__getstate__())
        state.pop("_i8_cache", None)
        state.pop("_similar_cache", None)
        return state

    def _similar_tables(self) -> dict:
        """The derived copies similar_items runs on, cached with the table and keyed on its identity and _version as
        int8_table is: "rows", the table itself or, where F is no multiple of 4, a copy with zero-padded rows (the
        scoring kernel reads 16 bytes at a time); "rnorm", the reciprocal row norms, filled on the first cosine call."""
        table = self._attr_table
        c = self.__dict__.get("_similar_cache")
        if c is None or c[0] is not table or c[1] != table._version:
            rows = table
            if table.shape[1] % 4 or table.data_ptr() % 16:
                rows = torch.zeros(table.shape[0], (table.shape[1] + 3) // 4 * 4, dtype=torch.float32, device=table.device)
                rows[:, :table.shape[1]] = table
            c = (table, table._version, dict(rows=rows, rnorm=None))
            self.__dict__["_similar_cache"] = c
        return c[2]

    def similar_items(self, items: Optional[Tensor] = None, k: int = 10, metric: str = "cosine", exclude_self: bool = True,
                      candidates=None, max_scratch_bytes: int = 1 << 30) -> Tuple[Tensor, Tensor]:
        """The k items whose attribute rows are closest to each listed item's: CARCA.similar_items over the registered
        attribute table [n_items, F] (its rows are the whole model), with the same arguments, order, padding and bits
        rules.  With metric "dot" and exclude_self=False the scores are recommend's for a profile ending in that item."""
        catalogue.similar_args("KNN.similar_items", items, k, metric)
        table = self._attr_table
        if table is None:
            raise CarcaHipError("KNN.similar_items: no attribute table registered -- call register_attr_table(attrs) with "
                                "the [n_items, n_attrs] item-attribute matrix first (the catalogue is its rows)")
        ops._need_cuda(table)
        with torch.no_grad():
            c = self._similar_tables()

            def rnorm():
                if c["rnorm"] is None:
                    c["rnorm"] = catalogue.row_rnorm(c["rows"], table.shape[1])
                return c["rnorm"]
            return catalogue.similar_items("KNN.similar_items", c["rows"], table.shape[1], rnorm, items, k, metric,
                                           exclude_self, candidates, max_scratch_bytes)

    def int8_table(self) -> Optional[Tensor]:
        """The int8 copy of the registered table that the catalogue scoring runs on (ops.knn_int8_table), or None when
        the table does not qualify.  Built on first use -- the only host sync -- and cached with the table, keyed on
        its identity and _version."""
        table = self._attr_table
        c = self.__dict__.get("_i8_cache")
        if c is None or c[0] is not table or c[1] != table._version:
            c = (table, table._version, ops.knn_int8_table(table))
            self.__dict__["_i8_cache"] = c
        return c[2]

    def recommend(self, profile: Tuple[Tensor, Optional[Tensor], Tensor], context: Optional[Tensor] = None, k: int = 10,
                  exclude="profile") -> Tuple[Tensor, Tensor]:
        """The k best items of the catalogue (the rows of the registered attribute table) per user: (scores [B, k]
        float32, ids [B, k] int64), best first.  The score of item i is forward's, attrs(last profile slot) . table[i]:
        the last slot's row of p_a when given, else table[p_x[:, -1]] (an id outside the table reads as a zero row).
        context is ignored (knn.py ignores it).  Order, exclusion ("profile", None or an int [B, E] tensor, 0 = no
        entry) and padding are CARCA.recommend's: ties go to the smaller id, id 0 is never listed, fewer than k
        eligible items pad with id 0 and score 0.  1 <= k <= 128; any L; train and eval mode alike."""
        return catalogue.recommend("KNN.recommend", _lib.KnnRecommendDesc, "carca_knn_recommend",
                                   lambda: catalogue.knn_model_side(self, profile, "KNN.recommend"), profile, k, exclude)

    def retrieve(self, profile: Tuple[Tensor, Optional[Tensor], Tensor], context: Optional[Tensor] = None, k: int = 1000,
                 exclude="profile") -> Tuple[Tensor, Tensor]:
        """recommend in depth: the k best items per user for 1 <= k <= catalogue.RETRIEVE_KMAX = 4096, with recommend's
        arguments, order, exclusion and padding; any L; train and eval mode alike.  retrieve(k)[:, :j] equals retrieve(j)
        bit for bit, retrieve(k) equals recommend(k) for k <= 128, and the scores are forward's / rank_items' for the
        returned pairs (CARCA.retrieve)."""
        return catalogue.retrieve("KNN.retrieve", _lib.KnnRecommendDesc, "carca_knn_retrieve",
                                  lambda: catalogue.knn_model_side(self, profile, "KNN.retrieve"), profile, k, exclude)

    def recommend_sampled(self, profile: Tuple[Tensor, Optional[Tensor], Tensor], context: Optional[Tensor] = None,
                          k: int = 10, temperature: float = 1.0, seed: Optional[int] = None,
                          user_keys: Optional[Tensor] = None, exclude="profile",
                          candidates=None) -> Tuple[Tensor, Tensor, Tensor]:
        """CARCA.recommend_sampled for the baseline: k items per user drawn without replacement from
        softmax(score / temperature) over the eligible rows of the registered table, (scores [B, k], ids [B, k],
        log_probs [B, k]), 1 <= k <= catalogue.RETRIEVE_KMAX, with its noise contract, seed, user_keys, padding and
        properties.  scores are KNN.recommend's raw dot products for the returned pairs, bit for
        bit; exclude is KNN.recommend's; candidates (None, a catalogue.CandidateSet or a 1-D id tensor / bool mask)
        strikes out every other item -- the whole catalogue is still scored.  Any L; train and eval mode alike."""
        return catalogue.recommend_sampled("KNN.recommend_sampled", _lib.KnnRecommendDesc, "carca_knn_recommend_sampled",
                                           lambda: catalogue.knn_model_side(self, profile, "KNN.recommend_sampled"),
                                           profile, k, temperature, seed, user_keys, exclude, candidates)

    def log_prob_items(self, profile: Tuple[Tensor, Optional[Tensor], Tensor], context: Optional[Tensor] = None,
                       items: Tensor = ..., temperature: float = 1.0, exclude="profile",
                       candidates=None) -> Tuple[Tensor, Tensor, Tensor]:
        """CARCA.log_prob_items for the baseline: (log_probs [B, N], lse [B], entropy [B]) of the listed items under
        softmax(score / temperature) over the eligible rows of the registered table, with its definitions, -inf for an
        ineligible entry, and independence of batch, list order and launch shape.  For the ids
        KNN.recommend_sampled returned under the same temperature, exclude and candidates, log_probs equals that call's
        bit for bit.  items (required; the default only keeps context optional) is an int [B, N] tensor.  Any L; train and
        eval mode alike."""
        if items is ...:
            raise CarcaHipError("KNN.log_prob_items: items is required: an int [B, N] tensor, one list per user")
        return catalogue.log_prob_items("KNN.log_prob_items", _lib.KnnRecommendDesc, "carca_knn_log_prob_items",
                                        lambda: catalogue.knn_model_side(self, profile, "KNN.log_prob_items"),
                                        profile, items, temperature, exclude, candidates)

    def recommend_diverse(self, profile: Tuple[Tensor, Optional[Tensor], Tensor], context: Optional[Tensor] = None,
                          k: int = 10, pool: int = 128, lam: float = 0.7, metric: str = "cosine", exclude="profile",
                          normalize: bool = True) -> Tuple[Tensor, Tensor, Tensor]:
        """CARCA.recommend_diverse for the baseline: recommend's `pool` best items re-ranked by maximal marginal relevance
        over the rows of the registered attribute table (the space similar_items measures in), with its cached reciprocal
        norms: (scores [B, k], ids [B, k] in selection order, ild [B]).  lam = 1 is recommend(k) bit for bit."""
        catalogue.mmr_args("KNN.recommend_diverse", k, pool, lam, metric)
        s, i = self.recommend(profile, context, k=pool, exclude=exclude)
        table = self._attr_table
        with torch.no_grad():
            c = self._similar_tables()

            def rnorm():
                if c["rnorm"] is None:
                    c["rnorm"] = catalogue.row_rnorm(c["rows"], table.shape[1])
                return c["rnorm"]
            return catalogue.mmr_rerank("KNN.recommend_diverse", s, i, c["rows"], table.shape[1], k, lam, metric, normalize,
                                        rnorm)

    def rank_items(self, profile: Tuple[Tensor, Optional[Tensor], Tensor], context: Optional[Tensor], items: Tensor,
                   exclude="profile") -> Tuple[Tensor, Tensor]:
        """Exact catalogue ranks of listed items: (scores [B, N] float32, ranks [B, N] int64), as CARCA.rank_items.
        items: an int32 / int64 [B, N] tensor, 1 <= N <= 128.  ranks[u, j] is the number of eligible items (id != 0,
        not excluded) before items[u, j] in recommend's order; an excluded or repeated item keeps its position.  Id 0
        or an id outside [0, n_items) gives rank -1 and score 0.  Scores and the order are bit-identical to
        recommend's; profile, context and exclude are recommend's."""
        return catalogue.rank_items("KNN.rank_items", _lib.KnnRankDesc, "carca_knn_rank_items",
                                    lambda: catalogue.knn_model_side(self, profile, "KNN.rank_items"), profile, items,
                                    exclude)

    def forward(self, profile: Tuple[Tensor, Tensor, Tensor], targets: List[Tuple[Tensor, Tensor, Tensor]]) -> Tensor:
        p_x, p_a, p_c = profile
        ys = []
        for o_x, o_a, o_c in targets:
            if p_a is None or o_a is None:
                if self._attr_table is None:
                    raise ValueError("KNN: attribute tensors are None and no table is registered (register_attr_table)")
                ys.append(ops.knn_score(None, None, p_x, o_x, table=self._attr_table))
            else:
                ys.append(ops.knn_score(p_a, o_a))
        return torch.cat(ys, dim=-1)  # knn.py:21


# ------------------------------------------------------------------------------------------------
# loss (carca.py:437-444)
# ------------------------------------------------------------------------------------------------


class BinaryCrossEntropy(nn.Module):
    def forward(self, y_pred: Tensor, y_true: Tensor, mask: Tensor, eps: float = 1e-8,
                denom: Optional[Tensor] = None) -> Tensor:
        """`denom` (extension, device float[1]): the whole batch's mask count when users are sharded (dist.py)."""
        if torch.is_grad_enabled() and y_pred.requires_grad:
            from .autograd import bce_with_grad

            return bce_with_grad(y_pred, y_true, mask, eps, denom)
        loss, _ = ops.bce_fwd(y_pred, y_true, mask != 0, eps, denom=denom)
        return loss
