"""Host side of the full-catalogue top-k and rank calls (CARCA.recommend / rank_items, KNN.recommend / rank_items;
DESIGN.md sections 10-12).  A call checks its arguments, builds the model side (carca_model_side or knn_model_side: a
ModelSide, what scores a (user, item) pair), asks it for a descriptor (ModelSide.desc) and does what the calls share --
the exclusion list, the outputs and the launch (recommend, rank_items).  A model's descriptors name their model-side
fields alike (include/carca_hip.h), so one side fills any of them.  CandidateSet is the item set the CARCA calls can be
restricted to.  similar_items is the item-to-item top-k over a row table (CARCA.similar_items,
KNN.similar_items, ops.similar_rows).  mmr_rerank is the diversity re-rank of a top-k pool over such a table
(recommend_diverse, ops.mmr_rerank).  score_items / recommend_from serve a candidate list of its
own per user (CARCA.score_items / recommend_from).  explain_items / explain_top_slots /
recommend_explained say which profile slots drive a cross-attention score.  ItemGroups labels
items with a group; recommend_by_group / recommend_capped are the top-k of every group and the top-k with a cap per group
(CARCA.recommend_by_group / recommend_capped).  AudienceTopK / recommend_users turn the question
round: the k best users of each listed item, kept across batches (CARCA.recommend_users, train.audience; DESIGN.md
section 24).  score_items_at / best_context / recommend_at serve several request contexts per user from one run of the
profile side (CARCA.score_items_at / best_context / recommend_at).  retrieve is recommend in
depth, k up to RETRIEVE_KMAX: the first stage those second-stage calls sit behind (CARCA.retrieve, KNN.retrieve; DESIGN.md
section 26).  recommend_sampled draws the list instead of sorting it -- Gumbel top-k over softmax(logit / temperature),
with each drawn item's log-probability -- and plackett_luce_log_prob turns those into the list's conditional
log-probabilities (CARCA.recommend_sampled, KNN.recommend_sampled)."""
from __future__ import annotations

import ctypes as C
import math
from types import SimpleNamespace
from typing import Callable, Optional, Tuple

import torch
from torch import Tensor

from . import _lib, ops
from ._lib import CarcaHipError

KMAX = 128  # largest k of recommend and largest list of rank_items (csrc: rc::RC_KMAX, rc::LIST_MAX)


def _check_k(what: str, k: int) -> int:
    if not 1 <= int(k) <= KMAX:
        raise CarcaHipError(f"{what}: k = {k} outside 1..{KMAX} (the largest k the selection keeps is {KMAX})")
    return int(k)


class CandidateSet:
    """A set S of item ids that CARCA.recommend / rank_items and train.evaluate_full / evaluate_full_ranks can be restricted
    to ("among these items"), shared by every user of a batch.

    items: a 1-D integer tensor of ids, in any order -- duplicates, zeros and ids outside [1, n_items) are dropped -- or a
    bool mask [n_items] (entry 0, the padding item, is ignored).  The constructor normalises once (sort, unique, range
    filter), which is the set's only host sync; build it once and reuse it across calls.  `ids` is the result: int32 [C],
    ascending and distinct, on `device` (default: where `items` lives); `n_items` the catalogue size it was built for.
    C = 0 is a legal set."""

    def __init__(self, items: Tensor, n_items: int, device=None):
        n_items = int(n_items)
        if n_items < 1:
            raise CarcaHipError(f"CandidateSet: n_items = {n_items} must be positive")
        if not isinstance(items, Tensor) or items.dim() != 1 or items.is_floating_point() or items.is_complex():
            raise CarcaHipError("CandidateSet: items must be a 1-D integer tensor of ids or a bool mask [n_items]")
        if items.dtype == torch.bool:
            if items.shape[0] != n_items:
                raise CarcaHipError(f"CandidateSet: a mask must have n_items = {n_items} entries, got {items.shape[0]}")
            ids = torch.nonzero(items, as_tuple=False).reshape(-1)
        else:
            ids = torch.unique(items.to(torch.int64))  # (sorted ascending)
        ids = ids[(ids >= 1) & (ids < n_items)]
        self.n_items = n_items
        self.ids = ids.to(dtype=torch.int32, device=items.device if device is None else device).contiguous()

    def __len__(self) -> int:
        return self.ids.shape[0]

    def to(self, device) -> "CandidateSet":
        """The set on `device`: itself when it is there already, else a copy of the normalised ids (no host sync)."""
        ids = self.ids.to(device)
        if ids is self.ids:
            return self
        out = object.__new__(CandidateSet)
        out.n_items, out.ids = self.n_items, ids
        return out

    def contains(self, ids: Tensor) -> Tensor:
        """Membership of each id of an integer tensor on the set's device, as a bool tensor of its shape (no host sync)."""
        C_ = self.ids.shape[0]
        if C_ == 0:
            return torch.zeros_like(ids, dtype=torch.bool)
        q = ids.to(torch.int64).clamp(-1, self.n_items).to(torch.int32).contiguous()
        at = torch.searchsorted(self.ids, q).clamp(max=C_ - 1)
        return self.ids[at] == q


def _candidates(what: str, candidates, D, keep: list, device):
    """candidates (None, a CandidateSet, or a raw tensor: a CandidateSet built for this call, one host sync) -> None or the
    CarcaCandidates struct of the launch."""
    if candidates is None:
        return None
    if not isinstance(candidates, CandidateSet):
        if not isinstance(candidates, Tensor):
            raise CarcaHipError(f"{what}: candidates must be None, a CandidateSet or a 1-D integer / bool tensor")
        candidates = CandidateSet(candidates, D.n_items, device=device)
    if candidates.n_items != D.n_items:
        raise CarcaHipError(f"{what}: the candidate set was built for n_items = {candidates.n_items}, the model has "
                            f"{D.n_items}")
    ids = candidates.to(device).ids
    ops._need_cuda(ids)
    keep.append(ids)
    return _lib.Candidates(ids.data_ptr() if ids.shape[0] else None, ids.shape[0])


class NegativeLists:
    """A list of negative item ids per group of rows, for ops.listed_xent / CARCA.listed_softmax_loss (DESIGN.md section
    30): hard negatives from CARCA.retrieve, logged impressions, any per-user candidate list.

    lists: an integer tensor [G, N], N >= 1, G N < 2^31; ids outside [1, n_items) -- 0 and negatives included -- are padding
    (no class), duplicates inside a list and across lists are allowed and each counts.  bias: None or a float [G, N]
    tensor added to the entries' logits (a logQ-style correction; no gradient).  The constructor builds once, on the
    lists' device (CPU tensors too), what the loss needs at every call; the read of U is its one host sync, so build it
    once per set of lists, not inside a captured step.  The fields: `lists` [G, N] int32 (ids outside [0, n_items) sent
    to -1 or n_items), `ids` [U] int32, the distinct live ids ascending (the rows of S the caller embeds), `index` [G, N]
    int32, the position in `ids` of each entry or -1 for padding, `csr_off` [U + 1] and `csr_ent` [G N] int32, the lists
    by item: csr_ent[csr_off[u] : csr_off[u + 1]] are the flat positions g N + j of the entries of ids[u], ascending (the
    fixed order in which the backward sums an item's gradient; ops.listed_csr), `bias` float32 [G, N] or None; n_items,
    G and N are ints.  An all-padding object is legal: U = 0."""

    def __init__(self, lists: Tensor, n_items: int, bias: Optional[Tensor] = None):
        n_items = int(n_items)
        if n_items < 1:
            raise CarcaHipError(f"NegativeLists: n_items = {n_items} must be positive")
        if not isinstance(lists, Tensor) or lists.dim() != 2 or lists.shape[0] < 1 or lists.shape[1] < 1 or \
                lists.is_floating_point() or lists.is_complex() or lists.dtype == torch.bool:
            raise CarcaHipError("NegativeLists: lists must be an integer tensor [G, N] with G, N >= 1")
        G, N = lists.shape
        if G * N >= 2 ** 31:
            raise CarcaHipError(f"NegativeLists: G x N = {G * N} must stay below 2^31")
        if bias is not None:
            if not isinstance(bias, Tensor) or tuple(bias.shape) != (G, N) or not bias.is_floating_point():
                raise CarcaHipError(f"NegativeLists: bias must be a float tensor [G, N] = [{G}, {N}]")
            bias = bias.detach().to(device=lists.device, dtype=torch.float32).contiguous()
        flat = lists.detach().reshape(-1).to(torch.int64)
        live = (flat >= 1) & (flat < n_items)
        safe = torch.where(live, flat, torch.zeros_like(flat))
        present = torch.zeros(n_items, dtype=torch.bool, device=lists.device)
        present[safe] = True
        present[0] = False
        ids = torch.nonzero(present, as_tuple=False).reshape(-1)  # (ascending; the one host sync: U)
        rank = torch.cumsum(present.to(torch.int64), 0) - 1
        index = torch.where(live, rank[safe], torch.full_like(flat, -1)).to(torch.int32).reshape(G, N).contiguous()
        self.n_items, self.G, self.N = n_items, G, N
        self.lists = flat.clamp(min=-1, max=n_items).to(torch.int32).reshape(G, N).contiguous()
        self.ids = ids.to(torch.int32).contiguous()
        self.index = index
        self.csr_off, self.csr_ent = ops.listed_csr(index, self.ids.shape[0])
        self.bias = bias

    def __len__(self) -> int:
        return self.ids.shape[0]

    _FIELDS = ("lists", "ids", "index", "csr_off", "csr_ent")

    def to(self, device) -> "NegativeLists":
        """The lists on `device`: itself when they are there already, else a copy of the built fields (no host sync)."""
        ids = self.ids.to(device)
        if ids is self.ids:
            return self
        out = object.__new__(NegativeLists)
        out.n_items, out.G, out.N = self.n_items, self.G, self.N
        for f in self._FIELDS:
            setattr(out, f, getattr(self, f).to(device))
        out.bias = None if self.bias is None else self.bias.to(device)
        return out


GROUPS_MAX = 65535  # most groups of an ItemGroups (csrc: RG_MAX_GROUPS, a grid dimension)
CAPPED_SCRATCH_MAX = 1 << 30  # bytes of recommend_capped's [B, G, m] key scratch (csrc: RG_MAX_KEY_BYTES)


class ItemGroups:
    """A group label per item (category, brand, price band, shelf) for CARCA.recommend_by_group / recommend_capped
    (DESIGN.md section 23), shared by every user of a batch.

    group_of: a 1-D integer tensor [n_items]; entry i is the group of item i, in [0, G).  A negative entry puts the item in
    no group: the two calls never return it.  Entry 0 (the padding item) is ignored.  G = n_groups when given (an entry
    >= G raises), else the largest label + 1; empty groups are legal, 1 <= G <= GROUPS_MAX.  The constructor normalises
    once, on the host -- the copy of group_of to the host is its only sync -- so build it once and reuse it across calls.
    The fields, all int32 and contiguous on `device` (default: where group_of lives): `order` [C], the grouped ids sorted by
    (group, id); `offsets` [G + 1], group g owning order[offsets[g]:offsets[g + 1]]; `pos_of` [n_items], the position of an
    id in order or -1; `group_of` [n_items], normalised: -1 for ungrouped items and for id 0.  n_items and n_groups are
    ints."""

    def __init__(self, group_of: Tensor, n_groups: Optional[int] = None, device=None):
        if not isinstance(group_of, Tensor) or group_of.dim() != 1 or group_of.is_floating_point() or \
                group_of.is_complex() or group_of.dtype == torch.bool or group_of.shape[0] < 1:
            raise CarcaHipError("ItemGroups: group_of must be a 1-D integer tensor [n_items] of group labels")
        n_items = group_of.shape[0]
        g = group_of.detach().to("cpu", torch.int64).clamp(min=-1)  # (the only host sync; clamp copies: group_of is kept)
        g[0] = -1
        top = int(g.max())
        if n_groups is None:
            G = max(top + 1, 1)
        else:
            G = int(n_groups)
            if G < 1:
                raise CarcaHipError(f"ItemGroups: n_groups = {G} must be positive")
            if top >= G:
                raise CarcaHipError(f"ItemGroups: group label {top} outside [0, n_groups = {G})")
        if G > GROUPS_MAX:
            raise CarcaHipError(f"ItemGroups: {G} groups exceed {GROUPS_MAX} (the selection launches one grid row per group)")
        keys, perm = torch.sort(torch.where(g < 0, G, g), stable=True)  # (group, id): ids ascend inside a group
        n_grouped = int((g >= 0).sum())
        order = perm[:n_grouped]
        offsets = torch.searchsorted(keys[:n_grouped].contiguous(), torch.arange(G + 1))
        pos_of = torch.full((n_items,), -1, dtype=torch.int64)
        pos_of[order] = torch.arange(n_grouped)
        device = group_of.device if device is None else device
        self.n_items, self.n_groups = n_items, G
        self._bounds = offsets.tolist()  # host copy: members() slices without a sync
        self.order, self.offsets, self.pos_of, self.group_of = (
            t.to(dtype=torch.int32, device=device).contiguous() for t in (order, offsets, pos_of, g))

    def __len__(self) -> int:
        return self.order.shape[0]

    def to(self, device) -> "ItemGroups":
        """The groups on `device`: itself when they are there already, else a copy of the normalised fields (no host
        sync)."""
        order = self.order.to(device)
        if order is self.order:
            return self
        out = object.__new__(ItemGroups)
        out.n_items, out.n_groups, out._bounds, out.order = self.n_items, self.n_groups, self._bounds, order
        out.offsets, out.pos_of, out.group_of = self.offsets.to(device), self.pos_of.to(device), self.group_of.to(device)
        return out

    def members(self, g: int) -> Tensor:
        """The ids of group g: its slice of `order`, ascending -- a valid CandidateSet argument (no host sync)."""
        if not 0 <= int(g) < self.n_groups:
            raise CarcaHipError(f"ItemGroups.members: group {g} outside [0, {self.n_groups})")
        return self.order[self._bounds[int(g)]:self._bounds[int(g) + 1]]


def check_groups(what: str, groups, n_items: Optional[int]) -> None:
    """groups is an ItemGroups and, where the catalogue size is known, was built for it."""
    if not isinstance(groups, ItemGroups):
        raise CarcaHipError(f"{what}: groups must be a catalogue.ItemGroups")
    if n_items is not None and groups.n_items != n_items:
        raise CarcaHipError(f"{what}: the item groups were built for n_items = {groups.n_items}, the model has {n_items}")


def _groups(what: str, groups: ItemGroups, D, keep: list, device):
    """-> the CarcaItemGroups struct of the launch."""
    check_groups(what, groups, D.n_items)
    gr = groups.to(device)
    ops._need_cuda(gr.order, gr.offsets, gr.pos_of)
    keep += [gr.order, gr.offsets, gr.pos_of]
    return _lib.ItemGroups(gr.order.data_ptr() if len(gr) else None, gr.offsets.data_ptr(), gr.pos_of.data_ptr(), len(gr),
                           gr.n_groups)


def grouped_args(what: str, groups, k: int, max_per_group: int = 1, n_items: Optional[int] = None) -> None:
    """The argument checks of recommend_by_group / recommend_capped that need no launch."""
    _check_k(what, k)
    if int(max_per_group) < 1:
        raise CarcaHipError(f"{what}: max_per_group = {max_per_group} must be positive")
    check_groups(what, groups, n_items)


def recommend_by_group(what: str, model_side: Callable, profile, groups: ItemGroups, k: int, exclude,
                       n_items: Optional[int] = None) -> Tuple[Tensor, Tensor]:
    """The k best items of every group per user (carca_recommend_groups): (scores [B, G, k] float32, ids [B, G, k] int64).
    model_side() -> the ModelSide; n_items: the model's catalogue size where the caller knows it without a launch (checked
    before the model side runs)."""
    grouped_args(what, groups, k, 1, n_items)
    with torch.no_grad():
        D, keep = _topk_desc(what, model_side(), k, exclude)
        device = profile[0].device
        gr = _groups(what, groups, D, keep, device)
        outs = _outputs(D, "ids_out", (D.B, groups.n_groups, D.k), device)
        _lib.check(_lib.load().carca_recommend_groups(C.byref(D), C.byref(gr), ops._stream()), what)
        return outs


def recommend_capped(what: str, model_side: Callable, profile, groups: ItemGroups, k: int, max_per_group: int, exclude,
                     n_items: Optional[int] = None) -> Tuple[Tensor, Tensor]:
    """The k best grouped items per user with at most max_per_group of any one group (carca_recommend_capped):
    (scores [B, k] float32, ids [B, k] int64)."""
    grouped_args(what, groups, k, max_per_group, n_items)
    m = min(int(k), int(max_per_group))
    B = profile[0].shape[0]
    if B * groups.n_groups * m * 8 > CAPPED_SCRATCH_MAX:
        raise CarcaHipError(f"{what}: B = {B} users x G = {groups.n_groups} groups x m = {m} per group: the key scratch "
                            f"of {B * groups.n_groups * m * 8} bytes exceeds {CAPPED_SCRATCH_MAX} (split the batch)")
    with torch.no_grad():
        D, keep = _topk_desc(what, model_side(), k, exclude)
        device = profile[0].device
        gr = _groups(what, groups, D, keep, device)
        outs = _outputs(D, "ids_out", (D.B, D.k), device)
        _lib.check(_lib.load().carca_recommend_capped(C.byref(D), C.byref(gr), m, ops._stream()), what)
        return outs


def carca_route(what: str, d: int, encoder_heads, L: int, decoder_heads: Optional[int], allow_composed: bool) -> str:
    """The envelope of CARCA.recommend / rank_items and the path their profile side takes: "fused" (the per-user kernels)
    or "composed" (long_profile's row-level encoder); raises CarcaHipError outside the envelope.  encoder_heads: H of every
    encoder block; decoder_heads: H of a cross-attention decoder, None for the dot decoders (their sweep needs only d).
    allow_composed=False: L <= 64 and every attention module's (d, H) among the built geometries, always fused.
    allow_composed=True: L <= 1024 and d <= 128; a cross-attention decoder still needs its own (d, H) built (the sweep's
    scorer is instantiated per geometry); the profile side is composed where ops.use_composed says so (L > 64, or an
    encoder head count with no fused geometry) and fused otherwise.  No tensor is touched."""
    heads = list(encoder_heads) + ([decoder_heads] if decoder_heads is not None else [])
    no_kernel = "(d, H) = ({}, {}) has no fused attention kernel built (CARCA_ATT_GEOMETRIES in csrc/attn_common.h)"
    if not allow_composed:
        if L > _lib.MAX_L:
            raise CarcaHipError(f"{what}: profile length L = {L} exceeds CARCA_MAX_L = {_lib.MAX_L} (allow_composed=True "
                                f"takes up to {_lib.MAX_PROFILE_L} slots)")
        bad = [H for H in heads if d > ops.FUSED_MAX_D or not ops.attn_geometry_built(d, H)]
        if bad:
            raise CarcaHipError(f"{what}: " + no_kernel.format(d, bad[0]))
        return "fused"
    if L > _lib.MAX_PROFILE_L:
        raise CarcaHipError(f"{what}: profile length L = {L} exceeds CARCA_MAX_PROFILE_L = {_lib.MAX_PROFILE_L}")
    if d > ops.FUSED_MAX_D:
        raise CarcaHipError(f"{what}: d = {d} exceeds {ops.FUSED_MAX_D} (the sweep keeps an item's row in registers)")
    if decoder_heads is not None and not ops.attn_geometry_built(d, decoder_heads):
        raise CarcaHipError(f"{what}: " + no_kernel.format(d, decoder_heads))
    return "composed" if ops.use_composed(d, encoder_heads, L) else "fused"


def _context_stages(model, M: Tensor, n_ctx: int) -> list:
    """The row products through which a request context enters a score, as (result, operand, weight, N, K, out_ld) in
    the order they run: M c; for a cross-attention decoder dq = (M c) W_Q^T, and w_ffn . M c where it has its residual."""
    from .modules import CrossAttentionBlock

    dec, d = model.decoder, model.embeds.d
    ld = ops.row_ld(d)
    stages = [("mc", "context", M, d, n_ctx, ld)]
    if isinstance(dec, CrossAttentionBlock):
        stages.append(("dq", "mc", dec.attn.WQ.weight.detach(), d, d, ld))  # (M c_u) W_Q^T
        if dec.residual:
            stages.append(("off", "mc", dec.ffn.weight.detach(), 1, d, 4))  # w_ffn . M c_u
    return stages


def carca_context_rows(model, M: Tensor, context: Tensor) -> Tuple[Tensor, Optional[Tensor], Optional[Tensor]]:
    """One request context per user, context [B, n_ctx] -> (M c [B, ld]; dq [B, ld] or None; w_ffn . M c [B, 4] or None):
    _context_stages, one row product each."""
    rows = {"context": ops._f32(context)}
    for name, src, w, N, K, out_ld in _context_stages(model, M, context.shape[-1]):
        (rows[name],) = ops.gemm_rows([dict(a0=rows[src])], w, N, K, out_ld)
    return rows["mc"], rows.get("dq"), rows.get("off")


def carca_context_rows_at(model, M: Tensor, by_context: Tensor) -> Tuple[Tensor, Optional[Tensor], Optional[Tensor]]:
    """C request contexts per user, by_context [C, B, n_ctx] dense -> carca_context_rows' three results stacked over the
    contexts, [C, B, ld] each.  The row product picks its kernel by shape, so a stage is NOT one [C * B, K] product: it is
    C products, each with the descriptor carca_context_rows builds for a [B, K] operand -- built once, its operand and
    output pointers advanced per context -- handed to carca_gemm_rows_group, which chooses a kernel per product as
    carca_gemm_rows does and lets those that choose the narrow kernel share launches (the same body over the same shapes:
    the single-context call's bits, four products to a launch)."""
    n_c = by_context.shape[0]
    rows = {"context": by_context}
    lib, stream = _lib.load(), ops._stream()
    for name, src, w, N, K, out_ld in _context_stages(model, M, by_context.shape[-1]):
        a = rows[src]
        out = torch.empty(n_c, a.shape[1], out_ld, dtype=torch.float32, device=a.device)
        D0, _, keep = ops._gemm_desc([dict(a0=a[0], out=out[0])], w, N, K, out_ld)
        arr = (_lib.GemmDesc * n_c)()
        for c in range(n_c):
            arr[c] = D0
            arr[c].seg[0].a0 = a.data_ptr() + 4 * c * a.stride(0)
            arr[c].seg[0].c = out.data_ptr() + 4 * c * out.stride(0)
        _lib.check(lib.carca_gemm_rows_group(arr, n_c, stream), "context rows")
        rows[name] = out
    return rows["mc"], rows.get("dq"), rows.get("off")


class ModelSide(SimpleNamespace):
    """What scores a (user, item) pair, as a value: the result of carca_model_side, carca_model_side_at and
    knn_model_side, built from keywords.  `fields`: the model-side fields of the model's descriptors that are set, by
    their header names (CARCA: B, L, n_items, d, H, decoder, the pointers and their ld_; KNN: B, L, n_items, F and the
    _KNN_MODEL names).  `p_ids`: the profile ids as int32.  `contexts`: the filled CarcaContexts of the _at form, else
    None.  Every other attribute is a tensor the pointers point into, by name -- CARCA: T, p_n, then qt, wt, kk, uu
    (cross-attention) or rows (the dot decoders' scored rows), and mc, dq, off where a context enters; KNN: table, and q
    or table_i8.  The side owns them: holding it keeps them alive, and a caller holds it until its launch is queued.  No
    call writes into a side, so one side fills any number of descriptors."""
    contexts = None

    def desc(self, cls):
        """A zeroed descriptor of class cls with the model-side fields set.  A class that lacks one of them raises: a
        KNN side does not go into a CARCA descriptor."""
        D = cls(**self.fields)
        if vars(D):  # (ctypes keeps a keyword that names no field as a plain attribute of the instance)
            raise CarcaHipError(f"{cls.__name__} has no field {sorted(vars(D))[0]}: this model side does not fit it")
        return D


def _carca_envelope(model, profile, what: str, allow_composed: bool) -> str:
    """The envelope of the CARCA calls (carca_route, a covered decoder) -> the route.  No tensor is touched."""
    from .modules import CrossAttentionBlock, DotProduct, WeightedDotProduct

    dec = model.decoder
    ca = isinstance(dec, CrossAttentionBlock)
    route = carca_route(what, model.embeds.d, [b.attn.H for b in model.encoder], profile[0].shape[1],
                        dec.attn.H if ca else None, allow_composed)
    if not ca and not isinstance(dec, (DotProduct, WeightedDotProduct)):
        raise CarcaHipError(f"{what}: decoder {type(dec).__name__} is not covered")
    return route


def _carca_context_free(model, profile, n_ctx: int, route: str) -> Tuple[ModelSide, Optional[Tensor]]:
    """Everything of a CARCA model side that reads no request context: the item-side tables from their
    per-weight-version caches, and the profile side -- the encoder path of forward (embed_segments, then the fused blocks +
    the final LayerNorm, or long_profile.encode where the route is composed), then K, V -> u or the dot decoders' scored
    last slot.  -> (the side, its context rows still null; the context matrix M, None where the embedding has none)."""
    from .modules import CrossAttentionBlock, WeightedDotProduct

    p_x, p_a, p_c = profile
    B, L = p_x.shape
    emb, dec = model.embeds, model.decoder
    d = emb.d
    ca = isinstance(dec, CrossAttentionBlock)
    T = emb.item_table()
    n_items = T.shape[0]
    M = emb.context_matrix(n_ctx)
    H = dec.attn.H if ca else model._heads()
    dpi, _, _ = ops.padded_dims(d, H)
    ld = ops.row_ld(d)
    # profile side: the encoder path of forward (embed_segments + the blocks + the final LayerNorm)
    es, _ = emb.embed_segments([(p_x, p_a, p_c, False)], ld_e=dpi)
    x = es[0]
    if route == "composed":  # the row-level kernels, as forward runs them for such a profile; rows padded back to dpi
        from . import long_profile
        from .autograd import _pad_to

        p_n = _pad_to(long_profile.encode(model, x[..., :d], p_x), dpi).view(B * L, dpi)
    else:
        for blk in model.encoder:
            blk._check_mode()
            x = ops.sa_block_fwd(x, p_x, blk.weights_struct(x.device), d, blk.attn.H, blk.residual)
        p_n = ops.layernorm_fwd(x.reshape(B * L, -1), model.norm.weight, model.norm.bias, d, dpi)
    p_ids = ops._ids32(p_x)
    f = dict(B=B, L=L, n_items=n_items, d=d, H=H, p_ids=p_ids.data_ptr(), ld_p_ids=L)
    if ca:
        qt, wt, wd = dec.recommend_tables(T)
        a = dec.attn
        (kk,) = ops.gemm_rows([dict(a0=p_n)], a.WK.weight.detach(), d, d, ld, bias=a.WK.bias.detach())
        (vv,) = ops.gemm_rows([dict(a0=p_n)], a.WV.weight.detach(), d, d, ld, bias=a.WV.bias.detach())
        (uu,) = ops.gemm_rows([dict(a0=vv)], wd, H, d, 4)  # u_lh = w_h . V_lh (the decoder FFN folded in)
        f.update(decoder=0, item_q=qt.data_ptr(), ld_item_q=qt.stride(0), user_k=kk.data_ptr(), ld_user_k=kk.stride(0),
                 user_u=uu.data_ptr(), ld_user_u=uu.stride(0), ffn_b=dec.ffn.bias.data_ptr())
        if dec.residual:
            f.update(item_w=wt.data_ptr(), ld_item_w=wt.stride(0))
        return ModelSide(fields=f, p_ids=p_ids, T=T, p_n=p_n, qt=qt, wt=wt, kk=kk, uu=uu), M
    rows = p_n
    f["decoder"] = 1
    if isinstance(dec, WeightedDotProduct):  # carca.py:385-389
        rows = ops.slot_decay_scale(p_n, B, L, d, dec.gamma, dpi)
        if dec.norm:
            rows = ops.l2norm_fwd(rows, d, dpi)
            f["decoder"] = 2
    last = rows.view(B, L, dpi)[:, L - 1]  # the last profile slot scores every candidate (carca.py:364,393)
    f.update(item_q=T.data_ptr(), ld_item_q=T.stride(0), user_q=last.data_ptr(), ld_user_q=last.stride(0))
    return ModelSide(fields=f, p_ids=p_ids, T=T, p_n=p_n, rows=rows), M


def carca_model_side(model, profile, context: Optional[Tensor], what: str, allow_composed: bool = False) -> ModelSide:
    """The model side of the CARCA calls under one request context per user, context [B, n_ctx] or None: the envelope
    checks (_carca_envelope), the share that reads no context (_carca_context_free), and last the rows through which the
    context enters a score, M c, dq and w . M c (carca_context_rows; side.mc, side.dq, side.off).  Call under no_grad."""
    ops._need_cuda(*profile, context)
    route = _carca_envelope(model, profile, what, allow_composed)
    n_ctx = context.shape[-1] if context is not None else 0
    if context is not None and tuple(context.shape) != (profile[0].shape[0], n_ctx):
        raise CarcaHipError(f"{what}: context must be [B, n_ctx], got {tuple(context.shape)}")
    side, M = _carca_context_free(model, profile, n_ctx, route)
    if M is not None:  # M c_u [B, d]: the context's share of every candidate's embedding
        side.mc, side.dq, side.off = mc, dq, off = carca_context_rows(model, M, context)
        if dq is not None:  # (a cross-attention decoder)
            side.fields.update(user_q=dq.data_ptr(), ld_user_q=dq.stride(0))
            if off is not None:
                side.fields.update(user_off=off.data_ptr(), ld_user_off=off.stride(0))
        else:
            side.fields.update(user_m=mc.data_ptr(), ld_user_m=mc.stride(0))
    return side


def knn_model_side(model, profile, what: str) -> ModelSide:
    """The model side of KNN.recommend / rank_items: the catalogue is the registered table [n_items, F] (fp32, contiguous
    rows) with its int8 copy where it qualifies (table mode only), the query p_a[:, L-1] when p_a is given (dense), else
    the table row of p_x[:, L-1]."""
    table = model._attr_table
    if table is None:
        raise CarcaHipError(f"{what}: no attribute table registered -- call register_attr_table(attrs) with the "
                            "[n_items, n_attrs] item-attribute matrix first (the catalogue is its rows)")
    p_x, p_a, _ = profile
    ops._need_cuda(table, p_x, p_a)
    B, L = p_x.shape
    n_items, F = table.shape
    p_ids = ops._ids32(p_x)
    f = dict(B=B, L=L, n_items=n_items, F=F, p_ids=p_ids.data_ptr(), ld_p_ids=p_ids.stride(0),
             table=table.data_ptr(), ld_table=table.stride(0))
    if p_a is not None:
        if p_a.dim() != 3 or p_a.shape[0] != B or p_a.shape[2] != F:
            raise CarcaHipError(f"{what}: p_a {tuple(p_a.shape)} does not match [B, L, F] = [{B}, {L}, {F}]")
        q = p_a[:, -1]
        if q.dtype != torch.float32 or q.stride(-1) != 1:
            q = q.to(torch.float32).contiguous()
        f.update(user_a=q.data_ptr(), ld_user_a=q.stride(0))
        return ModelSide(fields=f, p_ids=p_ids, table=table, q=q)
    table_i8 = model.int8_table()
    if table_i8 is not None:
        f.update(table_i8=table_i8.data_ptr(), ld_table_i8=table_i8.stride(0))
    return ModelSide(fields=f, p_ids=p_ids, table=table, table_i8=table_i8)


def _ids32_clamped(ids: Tensor, n_items: int) -> Tensor:  # (clamped first: no int64 id wraps into range on the way to int32)
    return ops._ids32(ids if ids.dtype == torch.int32 else ids.clamp(-1, n_items))


def _exclusion(what: str, exclude, p_ids: Tensor, D, clamp: bool) -> Optional[Tensor]:
    """exclude ("profile", None or an int [B, E] tensor) -> D.exclude / n_exclude / ld_exclude, and the int32 tensor they
    point into (None: no list), which the caller keeps.  clamp: as _ids32_clamped (the rank call; the top-k call casts as
    it always has, without the extra launch)."""
    if isinstance(exclude, str):
        if exclude != "profile":
            raise CarcaHipError(f'{what}: exclude must be "profile", None or an int [B, E] tensor')
        excl = p_ids
    elif exclude is None:
        return None
    else:
        ops._need_cuda(exclude)
        if exclude.dim() != 2 or exclude.shape[0] != D.B or exclude.is_floating_point():
            raise CarcaHipError(f"{what}: exclude must be an int [B, E] tensor")
        excl = _ids32_clamped(exclude, D.n_items) if clamp else ops._ids32(exclude)
    if excl.shape[1] == 0:
        return None
    D.exclude, D.n_exclude, D.ld_exclude = excl.data_ptr(), excl.shape[1], excl.stride(0)
    return excl


def _topk_desc(what: str, side: ModelSide, k: int, exclude, desc=_lib.RecommendDesc):
    """-> (side's descriptor of class desc with k and the exclusion list set; the list of what it points into, the side
    first, held by the call until its launch is queued)."""
    D = side.desc(desc)
    D.k = int(k)
    return D, [side, _exclusion(what, exclude, side.p_ids, D, clamp=False)]


def _outputs(D, second: Optional[str], shape, device) -> Tuple[Tensor, Tensor]:
    """Fresh outputs of `shape` (float32, int64), one row per user; D.scores and, where named, D.<second> point at them,
    their ld_ a user's row."""
    outs = (torch.empty(shape, dtype=torch.float32, device=device), torch.empty(shape, dtype=torch.int64, device=device))
    ld = math.prod(shape[1:])
    D.scores, D.ld_scores = outs[0].data_ptr(), ld
    if second is not None:
        setattr(D, second, outs[1].data_ptr())
        setattr(D, "ld_" + second, ld)
    return outs


def _launch(what: str, D, entry: str, second: str, n: int, device, cand=None) -> Tuple[Tensor, Tensor]:
    """Points D at fresh [B, n] outputs (_outputs) and queues the C entry point -- with a candidate list `cand`, its
    _among form."""
    outs = _outputs(D, second, (D.B, n), device)
    if cand is None:
        rc = getattr(_lib.load(), entry)(C.byref(D), ops._stream())
    else:
        rc = getattr(_lib.load(), entry + "_among")(C.byref(D), C.byref(cand), ops._stream())
    _lib.check(rc, what)
    return outs


def recommend(what: str, desc, entry: str, model_side: Callable, profile, k: int, exclude,
              candidates=None) -> Tuple[Tensor, Tensor]:
    """The top-k call: desc the descriptor class, entry its C entry point, model_side() -> the ModelSide, run after the
    argument checks; candidates: None, or the set the call is restricted to (entry + "_among")."""
    _check_k(what, k)
    return _topk(what, desc, entry, model_side, profile, k, exclude, candidates)


def _topk(what: str, desc, entry: str, model_side: Callable, profile, k: int, exclude, candidates) -> Tuple[Tensor, Tensor]:
    """What recommend and retrieve do once k has passed: the descriptor, the candidate list, the outputs, the launch."""
    with torch.no_grad():
        D, keep = _topk_desc(what, model_side(), k, exclude, desc)
        cand = _candidates(what, candidates, D, keep, profile[0].device)
        return _launch(what, D, entry, "ids_out", D.k, profile[0].device, cand)


RETRIEVE_KMAX = 4096  # largest k of retrieve (csrc: rc::DS_KMAX, the deep selection's LDS key block)


def retrieve(what: str, desc, entry: str, model_side: Callable, profile, k: int, exclude,
             candidates=None) -> Tuple[Tensor, Tensor]:
    """The deep top-k call: recommend's arguments, contract and launches but the selection, with
    1 <= k <= RETRIEVE_KMAX; entry: carca_retrieve or carca_knn_retrieve.  k is checked before model_side() runs."""
    if not 1 <= int(k) <= RETRIEVE_KMAX:
        raise CarcaHipError(f"{what}: k = {k} outside 1..{RETRIEVE_KMAX} (the largest k the deep selection keeps is "
                            f"{RETRIEVE_KMAX})")
    return _topk(what, desc, entry, model_side, profile, int(k), exclude, candidates)


# ---- Gumbel top-k sampling with logged propensities (include/carca_hip.h: CarcaSampling) ---------
FLT_MIN = 2.0 ** -126  # the smallest normal fp32 number: the smallest temperature (csrc: sp_check)


def sampled_args(what: str, profile, k: int, temperature, seed, user_keys) -> Tuple[int, float, int]:
    """The checks of recommend_sampled's own arguments, before any device work: -> (k, temperature, seed mod 2^64).
    temperature must be a finite float that is a normal positive number as fp32 (FLT_MIN <= t < inf); seed an int, or None: drawn from torch's CPU generator
    as the dropout seed is (ops.new_dropout_seed), so torch.manual_seed makes a call sequence reproducible; user_keys None
    or an int [B] tensor."""
    if not 1 <= int(k) <= RETRIEVE_KMAX:
        raise CarcaHipError(f"{what}: k = {k} outside 1..{RETRIEVE_KMAX} (the largest k the deep selection keeps is "
                            f"{RETRIEVE_KMAX})")
    if isinstance(temperature, bool) or not isinstance(temperature, (int, float)):
        raise CarcaHipError(f"{what}: temperature must be a finite float > 0, got {temperature!r}")
    t32 = C.c_float(float(temperature)).value  # (what the kernels divide by)
    if not (math.isfinite(t32) and t32 >= FLT_MIN):  # (a denormal would take logit / temperature to +-inf)
        raise CarcaHipError(f"{what}: temperature must be a finite float > 0, a normal fp32 number (>= {FLT_MIN:.3e}), "
                            f"got {temperature!r}")
    if seed is None:
        seed = ops.new_dropout_seed()
    elif isinstance(seed, bool) or not isinstance(seed, int):
        raise CarcaHipError(f"{what}: seed must be an int or None, got {seed!r}")
    if user_keys is not None:
        B = profile[0].shape[0]
        if not isinstance(user_keys, Tensor) or user_keys.is_floating_point() or user_keys.is_complex() or \
                user_keys.dtype == torch.bool or tuple(user_keys.shape) != (B,):
            raise CarcaHipError(f"{what}: user_keys must be None or an int [B] tensor with B = {B}")
    return int(k), t32, int(seed) % (1 << 64)


def recommend_sampled(what: str, desc, entry: str, model_side: Callable, profile, k: int, temperature, seed, user_keys,
                      exclude, candidates=None) -> Tuple[Tensor, Tensor, Tensor]:
    """The sampling call: recommend's arguments and eligibility, the list drawn without replacement
    from softmax(logit / temperature) by Gumbel top-k: -> (scores [B, k] float32, ids [B, k] int64, log_probs [B, k]
    float32).  entry: carca_recommend_sampled or carca_knn_recommend_sampled (both take a nullable candidate list).  Every
    argument of its own is checked (sampled_args) before model_side() runs."""
    k, t32, seed = sampled_args(what, profile, k, temperature, seed, user_keys)
    with torch.no_grad():
        D, keep = _topk_desc(what, model_side(), k, exclude, desc)
        device = profile[0].device
        cand = _candidates(what, candidates, D, keep, device)
        X = _lib.Sampling(temperature=t32, seed=seed)
        if user_keys is not None:
            ops._need_cuda(user_keys)
            keys = user_keys.to(torch.int64).contiguous()
            keep.append(keys)
            X.user_keys = keys.data_ptr()
        scores, ids = _outputs(D, "ids_out", (D.B, k), device)
        log_probs = torch.empty(D.B, k, dtype=torch.float32, device=device)
        X.log_probs, X.ld_log_probs = log_probs.data_ptr(), k
        rc = getattr(_lib.load(), entry)(C.byref(D), C.byref(cand) if cand is not None else None, C.byref(X), ops._stream())
        _lib.check(rc, what)
        return scores, ids, log_probs


def plackett_luce_log_prob(log_probs: Tensor) -> Tensor:
    """recommend_sampled's log_probs [B, k] -> the conditional log-probabilities [B, k] (float64) of the ordered list drawn
    without replacement: out[:, j] = lp_j - log1p(-sum_{m<j} exp(lp_m)), the log-probability of item j among the items
    that the first j draws left; out.sum(1) is the Plackett-Luce log-probability of the list.  Padding (-inf) stays -inf.
    Torch ops in float64 on the input's device; not a kernel.

    Cancellation: 1 - sum_{m<j} exp(lp_m) is the mass that is left, computed from fp32 log_probs whose absolute error is
    about 1e-6 at best.  When the drawn head holds nearly all the mass -- a cold temperature, or k close to the eligible
    count -- that difference loses its leading digits: with a remaining mass r the result's error grows like 1e-6 / r,
    and once the rounded head sums to 1 or more the remainder clamps at 0 and the entry is +inf (-inf where lp_j is
    itself -inf).  Trust column j only while the head's mass stays well below 1."""
    if not isinstance(log_probs, Tensor) or log_probs.dim() != 2 or not log_probs.is_floating_point():
        raise CarcaHipError("plackett_luce_log_prob: log_probs must be a float [B, k] tensor")
    lp = log_probs.to(torch.float64)
    p = torch.exp(lp)
    head = torch.cumsum(p, dim=1) - p  # sum_{m<j} exp(lp_m)
    out = lp - torch.log1p(-head.clamp(max=1.0))
    return torch.where(torch.isneginf(lp), lp, out)


# ---- a policy's log-probabilities for logged items (include/carca_hip.h: CarcaPolicyItems) -------
def policy_args(what: str, profile, items, temperature) -> float:
    """The checks of log_prob_items' own arguments, before any device work: -> the temperature as the fp32 value the
    kernels divide by.  temperature as sampled_args asks: a finite float that is a normal positive number as fp32; items
    an int [B, N] tensor, N >= 0."""
    if isinstance(temperature, bool) or not isinstance(temperature, (int, float)):
        raise CarcaHipError(f"{what}: temperature must be a finite float > 0, got {temperature!r}")
    t32 = C.c_float(float(temperature)).value
    if not (math.isfinite(t32) and t32 >= FLT_MIN):  # (a denormal would take logit / temperature to +-inf)
        raise CarcaHipError(f"{what}: temperature must be a finite float > 0, a normal fp32 number (>= {FLT_MIN:.3e}), "
                            f"got {temperature!r}")
    B = profile[0].shape[0]
    if not isinstance(items, Tensor) or items.dim() != 2 or items.is_floating_point() or items.is_complex() or \
            items.dtype == torch.bool or items.shape[0] != B:
        raise CarcaHipError(f"{what}: items must be an int [B, N] tensor, one row per user, with B = {B}")
    return t32


def log_prob_items(what: str, desc, entry: str, model_side: Callable, profile, items: Tensor, temperature, exclude,
                   candidates=None) -> Tuple[Tensor, Tensor, Tensor]:
    """The policy call: recommend_sampled's arguments and eligibility with a list per user in place
    of the draw: -> (log_probs [B, N] float32, lse [B] float32, entropy [B] float32).  entry: carca_log_prob_items or
    carca_knn_log_prob_items (both take a nullable candidate list).  The ids go to the kernel as int64, so no id wraps
    into range.  Every argument of its own is checked (policy_args) before model_side() runs."""
    t32 = policy_args(what, profile, items, temperature)
    with torch.no_grad():
        D, keep = _topk_desc(what, model_side(), 0, exclude, desc)
        device = profile[0].device
        cand = _candidates(what, candidates, D, keep, device)
        ops._need_cuda(items)
        N = items.shape[1]
        lst = items.to(torch.int64).contiguous()
        log_probs = torch.empty(D.B, N, dtype=torch.float32, device=device)
        lse = torch.empty(D.B, dtype=torch.float32, device=device)
        entropy = torch.empty(D.B, dtype=torch.float32, device=device)
        X = _lib.PolicyItems(temperature=t32, items=lst.data_ptr() if N else None, n_list=N, ld_items=N,
                             log_probs=log_probs.data_ptr() if N else None, ld_log_probs=N, lse=lse.data_ptr(),
                             entropy=entropy.data_ptr())
        rc = getattr(_lib.load(), entry)(C.byref(D), C.byref(cand) if cand is not None else None, C.byref(X), ops._stream())
        _lib.check(rc, what)
        return log_probs, lse, entropy


def policy_log_ratio(target_log_probs: Tensor, logged_log_probs: Tensor, mode: str = "first") -> Tensor:
    """log(pi_target / pi_logged) per logged row, [B] float64: the log of an importance weight.  target_log_probs: what
    log_prob_items returned for the logged ids under the policy being evaluated; logged_log_probs: what
    recommend_sampled logged; both [B, k].

    mode "first" takes column 0, the first draw -- the only position whose logged value is a true marginal (a later
    item's first-draw probability is not the probability that it was drawn there).  mode "list" takes the Plackett-Luce
    log-probability of the ordered list, plackett_luce_log_prob(.) summed over the columns that are not padding (-inf) in
    the LOGGED row, on either side; its cancellation caveat applies.

    A -inf target where the log is finite gives -inf: the target policy never takes that action, weight 0.  A finite
    target where the log says -inf raises: the logging policy cannot have drawn it (the log and the target disagree on
    eligibility -- another exclude or candidates).  The check is the function's one host sync.  Torch ops in float64 on
    the input's device; not a kernel."""
    ratio, bad = _policy_log_ratio(target_log_probs, logged_log_probs, mode)
    if bool(bad):
        raise CarcaHipError(_RATIO_UNDRAWN)
    return ratio


_RATIO_UNDRAWN = ("policy_log_ratio: a logged log-probability is -inf where the target's is finite: the logging policy "
                  "cannot have drawn that item (the log and the target disagree on eligibility)")


def _policy_log_ratio(target_log_probs: Tensor, logged_log_probs: Tensor, mode: str) -> Tuple[Tensor, Tensor]:
    """policy_log_ratio without its host sync: -> (the ratio [B] float64; a 0-d bool tensor, true where the raising case
    occurred, for the caller to test when it syncs)."""
    for name, t in (("target_log_probs", target_log_probs), ("logged_log_probs", logged_log_probs)):
        if not isinstance(t, Tensor) or t.dim() != 2 or not t.is_floating_point():
            raise CarcaHipError(f"policy_log_ratio: {name} must be a float [B, k] tensor")
    if target_log_probs.shape != logged_log_probs.shape:
        raise CarcaHipError(f"policy_log_ratio: shapes differ: target {tuple(target_log_probs.shape)}, logged "
                            f"{tuple(logged_log_probs.shape)}")
    if mode not in ("first", "list"):
        raise CarcaHipError(f'policy_log_ratio: mode must be "first" or "list", got {mode!r}')
    if target_log_probs.shape[1] < 1:
        raise CarcaHipError("policy_log_ratio: k = 0: no logged action")
    tgt, log = target_log_probs.to(torch.float64), logged_log_probs.to(torch.float64)
    if mode == "first":
        tgt, log = tgt[:, :1], log[:, :1]
    pad = torch.isneginf(log)
    bad = (pad & ~torch.isneginf(tgt)).any()
    if mode == "list":
        tgt, log = plackett_luce_log_prob(tgt), plackett_luce_log_prob(log)
    zero = torch.zeros((), dtype=torch.float64, device=log.device)
    return (torch.where(pad, zero, tgt) - torch.where(pad, zero, log)).sum(1), bad


def _off_policy_sums(log_ratio: Tensor, rewards: Tensor, clip) -> Tensor:
    """[sum w r, sum w, sum w^2, max w, n] float64 on the input's device, w = min(exp(log_ratio), clip)."""
    if not isinstance(log_ratio, Tensor) or log_ratio.dim() != 1 or not isinstance(rewards, Tensor) or \
            rewards.shape != log_ratio.shape:
        raise CarcaHipError("off_policy_estimate: log_ratio and rewards must be [B] tensors of one shape")
    if clip is not None and not (isinstance(clip, (int, float)) and not isinstance(clip, bool) and clip > 0):
        raise CarcaHipError(f"off_policy_estimate: clip must be None or a number > 0, got {clip!r}")
    w = torch.exp(log_ratio.to(torch.float64))
    if clip is not None:
        w = w.clamp(max=float(clip))
    r = rewards.to(device=w.device, dtype=torch.float64)
    n = torch.full((), float(w.shape[0]), dtype=torch.float64, device=w.device)
    peak = w.max() if w.shape[0] else torch.zeros((), dtype=torch.float64, device=w.device)
    return torch.stack([(w * r).sum(), w.sum(), (w * w).sum(), peak, n])


def _off_policy_result(sums: Tensor, clip) -> dict:
    wr, w1, w2, peak, n = sums.unbind(0)
    return dict(ips=wr / n, snips=wr / w1, ess=w1 * w1 / w2, max_weight=peak, n=n, clip=clip)


def off_policy_estimate(log_ratio: Tensor, rewards: Tensor, clip: Optional[float] = None) -> dict:
    """Inverse-propensity estimates of a target policy's value from logged rewards.  log_ratio [B]: policy_log_ratio's
    log weights; rewards [B]: the reward each logged row earned; w = exp(log_ratio), capped from above at clip when one is
    given (bias for variance).  -> dict of 0-d float64 tensors on log_ratio's device -- nothing is synced; the caller
    decides when -- and the clip:
      ips         mean of w r: unbiased when the logging policy covers the target's support and clip is None;
      snips       sum w r / sum w, the self-normalised estimate: biased, consistent, bounded by the rewards' range;
      ess         (sum w)^2 / sum w^2, the effective sample size: n when every weight is 1;
      max_weight  the largest (clipped) weight;
      n           the number of rows;
      clip        as given.
    No rows, or weights that are all 0, give nan where the formula divides by zero."""
    return _off_policy_result(_off_policy_sums(log_ratio, rewards, clip), clip)


# ---- objectives over a policy's differentiable log-probabilities -------------------------------
POLICY_OBJECTIVES = ("ips", "clipped_ips", "snips", "weighted_nll")
_OBJECTIVE_UNDRAWN = ("policy_objective: a logged log-probability is -inf on a valid row: the logging policy cannot have "
                      "drawn that item (the log and the policy disagree on eligibility)")


def _policy_objective(log_probs: Tensor, valid: Tensor, logged_log_probs: Optional[Tensor], rewards: Tensor, kind: str,
                      clip=None, entropy: Optional[Tensor] = None, entropy_coef: float = 0.0) -> Tuple[Tensor, Tensor]:
    """policy_objective without its host sync: -> (the loss, 0-d float64; a 0-d bool tensor, true where the raising case
    occurred, for the caller to test when it syncs)."""
    if kind not in POLICY_OBJECTIVES:
        raise CarcaHipError(f"policy_objective: kind must be one of {POLICY_OBJECTIVES}, got {kind!r}")
    if not isinstance(log_probs, Tensor) or not log_probs.is_floating_point():
        raise CarcaHipError("policy_objective: log_probs must be a float tensor")
    if not isinstance(valid, Tensor) or valid.shape != log_probs.shape:
        raise CarcaHipError("policy_objective: valid must have log_probs' shape")
    if not isinstance(rewards, Tensor) or rewards.shape != log_probs.shape:
        raise CarcaHipError("policy_objective: rewards must have log_probs' shape")
    if logged_log_probs is None:
        if kind != "weighted_nll":
            raise CarcaHipError(f'policy_objective: kind "{kind}" needs logged_log_probs')
    elif not isinstance(logged_log_probs, Tensor) or logged_log_probs.shape != log_probs.shape:
        raise CarcaHipError("policy_objective: logged_log_probs must have log_probs' shape")
    if kind == "clipped_ips":
        if not (isinstance(clip, (int, float)) and not isinstance(clip, bool) and clip > 0):
            raise CarcaHipError(f'policy_objective: kind "clipped_ips" needs a clip > 0, got {clip!r}')
    elif clip is not None:
        raise CarcaHipError('policy_objective: clip belongs to kind "clipped_ips"')
    if entropy_coef != 0.0 and (not isinstance(entropy, Tensor) or entropy.shape != log_probs.shape):
        raise CarcaHipError("policy_objective: a non-zero entropy_coef needs entropy with log_probs' shape")
    dev = log_probs.device
    ok = valid.to(device=dev) != 0
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    m = ok.to(torch.float64)
    n = m.sum().clamp(min=1.0)  # (no valid row: every sum below is 0, and so is the loss)
    lp = torch.where(ok, log_probs.to(torch.float64), zero)
    r = torch.where(ok, rewards.to(device=dev, dtype=torch.float64), zero)
    bad = torch.zeros((), dtype=torch.bool, device=dev)
    if logged_log_probs is not None:
        lg = logged_log_probs.to(device=dev, dtype=torch.float64)
        bad = (ok & torch.isneginf(lg)).any()
        lg = torch.where(ok, lg, zero)
    if kind == "weighted_nll":
        w0 = m if logged_log_probs is None else torch.exp(lp.detach() - lg) * m
        loss = -(r * w0 * lp).sum() / n
    else:
        w = torch.exp(lp - lg) * m
        if kind == "ips":
            loss = -(r * w).sum() / n
        elif kind == "clipped_ips":
            cap = torch.full((), float(clip), dtype=torch.float64, device=dev)
            loss = -(r * torch.where(w < cap, w, cap) * m).sum() / n  # (rows at the cap are constants: no gradient)
        else:
            ws = w.sum()
            loss = -(r * w).sum() / torch.where(ws > 0, ws, torch.ones_like(ws))
    if entropy_coef != 0.0:
        loss = loss - float(entropy_coef) * torch.where(ok, entropy.to(torch.float64), zero).sum() / n
    return loss, bad


def policy_objective(log_probs: Tensor, valid: Tensor, logged_log_probs: Optional[Tensor], rewards: Tensor, kind: str,
                     clip: Optional[float] = None, entropy: Optional[Tensor] = None, entropy_coef: float = 0.0) -> Tensor:
    """A loss to minimise over the valid rows of CARCA.log_prob_rows' output, 0-d float64, differentiable through
    log_probs and entropy.  log_probs, valid, logged_log_probs, rewards (and entropy) share one shape; logged_log_probs is
    what the logging policy reported for the same actions (recommend_sampled's column 0).  With w = exp(log_probs -
    logged) and means over the valid rows, kind is one of
      "ips"           -mean(r w): minus the inverse-propensity estimate of the policy's value;
      "clipped_ips"   -mean(r min(w, clip)): rows at the cap get no gradient;
      "snips"         -(sum r w) / (sum w): the self-normalised estimate;
      "weighted_nll"  -mean(r w_0 log_probs) with w_0 = 1 when logged_log_probs is None, else the detached weight
                      exp(log_probs.detach() - logged): reward-weighted likelihood.
    Every kind subtracts entropy_coef * mean(entropy).  No valid row gives 0 with zero gradients.  Rows that are not
    valid are read nowhere (their logged value and reward may be anything).  A valid row whose logged value is -inf
    raises: the logging policy cannot have drawn it; that check is the function's one host sync, as policy_log_ratio's
    (_policy_objective returns the flag instead, for a caller that syncs later).  Torch ops in float64 on log_probs'
    device; not a kernel."""
    loss, bad = _policy_objective(log_probs, valid, logged_log_probs, rewards, kind, clip, entropy, entropy_coef)
    if bool(bad):
        raise CarcaHipError(_OBJECTIVE_UNDRAWN)
    return loss


def off_policy_rows(shape, ids: Tensor, logged_log_probs: Tensor, rewards: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """A logged batch as log_prob_rows' rows: (items, logged, rewards), each [B, L] = shape, with the first logged column
    (ids[:, 0], its log-probability, its reward) at column L - 1 -- the policy after the whole profile -- and 0 elsewhere.
    Only that column's logged value is a true softmax marginal (section 28)."""
    B, L = shape
    if ids.dim() != 2 or ids.shape[0] != B or ids.shape[1] < 1 or logged_log_probs.shape != ids.shape:
        raise CarcaHipError(f"off_policy_step: ids and logged_log_probs must be [B = {B}, k >= 1] tensors of one shape")
    if rewards.shape[0] != B or rewards.dim() not in (1, 2):
        raise CarcaHipError(f"off_policy_step: rewards must be [B = {B}] or [B, k]")
    r = rewards[:, 0] if rewards.dim() == 2 else rewards
    items = torch.zeros(B, L, dtype=ids.dtype, device=ids.device)
    logged = torch.zeros(B, L, dtype=torch.float64, device=ids.device)
    rew = torch.zeros(B, L, dtype=torch.float64, device=ids.device)
    items[:, L - 1] = ids[:, 0]
    logged[:, L - 1] = logged_log_probs[:, 0].to(torch.float64)
    rew[:, L - 1] = r.to(device=ids.device, dtype=torch.float64)
    return items, logged, rew


def rank_items(what: str, desc, entry: str, model_side: Callable, profile, items: Tensor, exclude,
               candidates=None) -> Tuple[Tensor, Tensor]:
    """The rank call; the arguments are recommend's, with the [B, N] list in place of k."""
    ops._need_cuda(items)
    if items.dim() != 2 or items.is_floating_point() or items.shape[0] != profile[0].shape[0]:
        raise CarcaHipError(f"{what}: items must be an int [B, N] tensor")
    N = items.shape[1]
    if not 1 <= N <= KMAX:
        raise CarcaHipError(f"{what}: N = {N} items per user outside 1..{KMAX}")
    with torch.no_grad():
        side = model_side()
        D = side.desc(desc)
        keep = [side, _exclusion(what, exclude, side.p_ids, D, clamp=True)]
        lst = _ids32_clamped(items, D.n_items)
        _set_list(D, lst)
        cand = _candidates(what, candidates, D, keep, profile[0].device)
        return _launch(what, D, entry, "ranks", N, profile[0].device, cand)


# ---- a candidate list per user (include/carca_hip.h: carca_score_lists / carca_recommend_lists) --
LIST_FUSED_MAX = 1024  # longest list of the one-launch top-k (csrc: LS_FUSED_MAX); read at call time


def _lists(what: str, model_side: Callable, profile, items: Tensor, desc=_lib.ListsDesc):
    """The checks and the descriptor score_items and recommend_from share (desc: explain's, which carries the same list
    fields): -> (D, the ModelSide that model_side() built once the list passed, the lists as int32)."""
    if not isinstance(items, Tensor) or items.dim() != 2 or items.is_floating_point() or items.is_complex() or \
            items.dtype == torch.bool or items.shape[0] != profile[0].shape[0] or items.shape[1] < 1:
        raise CarcaHipError(f"{what}: items must be an int [B, N] tensor with N >= 1, one row per user")
    if items.shape[0] * items.shape[1] >= 2 ** 31:
        raise CarcaHipError(f"{what}: B * N = {items.shape[0] * items.shape[1]} does not fit an int")
    ops._need_cuda(items)
    side = model_side()
    D = side.desc(desc)
    return D, side, _ids32_clamped(items, D.n_items)


def _set_list(D, lst: Tensor) -> None:
    D.items, D.n_list, D.ld_items = lst.data_ptr(), lst.shape[1], lst.stride(0)


def score_items(what: str, model_side: Callable, profile, items: Tensor) -> Tensor:
    """The list-scoring call: scores [B, N] float32 of each user's own list, in caller order (carca_score_lists)."""
    with torch.no_grad():
        D, side, lst = _lists(what, model_side, profile, items)
        scores = torch.empty(D.B, lst.shape[1], dtype=torch.float32, device=profile[0].device)
        D.scores, D.ld_scores = scores.data_ptr(), lst.shape[1]
        _set_list(D, lst)
        _lib.check(_lib.load().carca_score_lists(C.byref(D), ops._stream()), what)
        return scores


def recommend_from(what: str, model_side: Callable, profile, items: Tensor, k: int, exclude) -> Tuple[Tensor, Tensor]:
    """The top-k call over each user's own list (carca_recommend_lists): a list of up to LIST_FUSED_MAX entries goes to
    the one-launch kernel as it is; a longer one is sorted per row on the device first (no host sync), which is the form
    the split path asks for."""
    k = _check_k(what, k)
    with torch.no_grad():
        D, side, lst = _lists(what, model_side, profile, items)
        D.k = k
        excl = _exclusion(what, exclude, side.p_ids, D, clamp=False)
        if lst.shape[1] > LIST_FUSED_MAX:
            lst = torch.sort(lst, dim=1).values
            D.sorted_rows = 1
        outs = _outputs(D, "ids_out", (D.B, k), profile[0].device)
        _set_list(D, lst)
        _lib.check(_lib.load().carca_recommend_lists(C.byref(D), ops._stream()), what)
        return outs


# ---- several request contexts per user (include/carca_hip.h: CarcaContexts) ---------------------
def contexts_args(what: str, single: str, profile, contexts) -> Tuple[int, int]:
    """The checks of `contexts` that touch no device: a float [B, C, n_ctx] tensor, C >= 1 -> (C, n_ctx).  single: the
    single-context call the messages name."""
    if not isinstance(contexts, Tensor) or contexts.dim() != 3 or not contexts.is_floating_point():
        raise CarcaHipError(f"{what}: contexts must be a float [B, C, n_ctx] tensor, the C request contexts of each user "
                            f"({single} takes one [B, n_ctx] context)")
    B = profile[0].shape[0]
    if contexts.shape[0] != B:
        raise CarcaHipError(f"{what}: contexts has {contexts.shape[0]} rows, the profile has B = {B} users")
    if contexts.shape[1] < 1:
        raise CarcaHipError(f"{what}: contexts holds C = 0 contexts per user; C must be at least 1")
    return contexts.shape[1], contexts.shape[2]


def carca_model_side_at(model, profile, contexts: Tensor, what: str, single: str,
                        allow_composed: bool = False) -> ModelSide:
    """carca_model_side for the C request contexts of each user, contexts [B, C, n_ctx] (contexts_args has checked it):
    the share that reads no context runs ONCE (_carca_context_free), and the context rows of every (user, context) pair
    (carca_context_rows_at) go to side.contexts, a filled CarcaContexts, as row u * C + c; the descriptors' own context
    rows stay null.  side.dq, side.off or side.mc are then [B, C, ld].  Two differences of envelope, both raised before
    anything is launched and naming `single`, the single-context call: an embedding without a context matrix, and a
    cross-attention decoder over more than CARCA_MAX_L slots."""
    from .modules import CrossAttentionBlock

    ops._need_cuda(*profile, contexts)
    L = profile[0].shape[1]
    if model.embeds.context_matrix(contexts.shape[2]) is None:
        raise CarcaHipError(f"{what}: {type(model.embeds).__name__} has no context matrix: its scores do not depend on the "
                            f"candidate's context, so every context gives what {single} gives (call {single})")
    if isinstance(model.decoder, CrossAttentionBlock) and L > _lib.MAX_L:
        raise CarcaHipError(f"{what}: profile length L = {L} exceeds CARCA_MAX_L = {_lib.MAX_L}: the chunked scorer of "
                            f"longer profiles is not served under several contexts (call {single} per context)")
    route = _carca_envelope(model, profile, what, allow_composed)
    side, M = _carca_context_free(model, profile, contexts.shape[2], route)
    by_context = ops._f32(contexts.transpose(0, 1))  # [C, B, n_ctx]: each context a dense [B, n_ctx] operand
    mc, dq, off = carca_context_rows_at(model, M, by_context)

    def by_user(t):  # [C, B, ld] -> [B, C, ld] dense: row u * C + c, row stride ld = shape[2] (C = 1: the same memory)
        return t.transpose(0, 1).contiguous()
    X = side.contexts = _lib.Contexts()
    X.n_contexts = contexts.shape[1]
    if dq is not None:  # (a cross-attention decoder)
        side.dq = dq = by_user(dq)
        X.user_q, X.ld_user_q = dq.data_ptr(), dq.shape[2]
        if off is not None:
            side.off = off = by_user(off)
            X.user_off, X.ld_user_off = off.data_ptr(), off.shape[2]
    else:
        side.mc = mc = by_user(mc)
        X.user_m, X.ld_user_m = mc.data_ptr(), mc.shape[2]
    return side


def _lists_at(what: str, model_side: Callable, profile, contexts: Tensor, items: Tensor):
    """_lists under several contexts, the list set: -> (D, the ModelSide, the lists as int32)."""
    n_c, _ = contexts_args(what, "score_items", profile, contexts)
    if isinstance(items, Tensor) and items.dim() == 2 and n_c * items.shape[1] >= 2 ** 31:
        raise CarcaHipError(f"{what}: C * N = {n_c * items.shape[1]} does not fit an int")
    D, side, lst = _lists(what, model_side, profile, items)
    _set_list(D, lst)
    return D, side, lst


def score_items_at(what: str, model_side: Callable, profile, contexts: Tensor, items: Tensor) -> Tensor:
    """score_items under each of a user's C contexts (carca_score_lists_at): scores [B, C, N] float32.  model_side() ->
    carca_model_side_at's ModelSide."""
    with torch.no_grad():
        D, side, lst = _lists_at(what, model_side, profile, contexts, items)
        X = side.contexts
        n_c, N = X.n_contexts, lst.shape[1]
        scores = torch.empty(D.B, n_c, N, dtype=torch.float32, device=profile[0].device)
        D.scores, D.ld_scores = scores.data_ptr(), n_c * N
        _lib.check(_lib.load().carca_score_lists_at(C.byref(D), C.byref(X), None, 0, ops._stream()), what)
        return scores


def best_context(what: str, model_side: Callable, profile, contexts: Tensor, items: Tensor) -> Tuple[Tensor, Tensor]:
    """Per (user, list entry) the context of the largest logit (carca_score_lists_at with best_context): (scores [B, N]
    float32, which [B, N] int64); no [B, C, N] buffer is formed."""
    with torch.no_grad():
        D, side, lst = _lists_at(what, model_side, profile, contexts, items)
        N = lst.shape[1]
        scores, which = _outputs(D, None, (D.B, N), profile[0].device)
        _lib.check(_lib.load().carca_score_lists_at(C.byref(D), C.byref(side.contexts), which.data_ptr(), N,
                                                    ops._stream()), what)
        return scores, which


def _user_rows(D, X, lo: int, hi: int):
    """Copies of a RecommendDesc and its CarcaContexts that cover users [lo, hi): every per-user pointer advanced by lo
    rows of its own stride (the exclusion list and the outputs hold C rows per user)."""
    n_c = X.n_contexts
    Dc, Xc = type(D).from_buffer_copy(D), type(X).from_buffer_copy(X)
    Dc.B = hi - lo
    for S, Sc, fields in ((D, Dc, (("p_ids", 4 * D.ld_p_ids), ("user_k", 4 * D.L * D.ld_user_k),
                                   ("user_u", 4 * D.L * D.ld_user_u), ("user_q", 4 * D.ld_user_q),
                                   ("exclude", 4 * n_c * D.ld_exclude), ("scores", 4 * D.ld_scores),
                                   ("ids_out", 8 * D.ld_ids_out))),
                          (X, Xc, (("user_q", 4 * n_c * X.ld_user_q), ("user_off", 4 * n_c * X.ld_user_off),
                                   ("user_m", 4 * n_c * X.ld_user_m)))):
        for name, row_bytes in fields:
            p = getattr(S, name)
            if p:
                setattr(Sc, name, p + lo * row_bytes)
    return Dc, Xc


def recommend_at(what: str, model_side: Callable, profile, contexts: Tensor, k: int, exclude, candidates=None,
                 max_scratch_bytes: int = 1 << 30) -> Tuple[Tensor, Tensor]:
    """recommend under each of a user's C contexts (carca_recommend_at / carca_recommend_among_at): (scores [B, C, k]
    float32, ids [B, C, k] int64).  model_side() -> carca_model_side_at's ModelSide.  The users go in chunks whose
    [users, C, n_slots] fp32 logit scratch stays within max_scratch_bytes, with no sync between them, each writing its
    rows of the outputs."""
    k = _check_k(what, k)
    n_c, _ = contexts_args(what, "recommend", profile, contexts)
    dev = profile[0].device
    with torch.no_grad():
        side = model_side()
        D, X = side.desc(_lib.RecommendDesc), side.contexts
        D.k = k
        excl = _exclusion(what, exclude, side.p_ids, D, clamp=False)
        if excl is not None and n_c > 1:  # user u's row for each of its contexts: row u * C + c of the launch's B * C users
            excl = excl.repeat_interleave(n_c, dim=0).contiguous()
            D.exclude, D.ld_exclude = excl.data_ptr(), excl.stride(0)
        keep = [side, excl]
        cand = _candidates(what, candidates, D, keep, dev)
        n_slots = D.n_items if cand is None else cand.n
        users = int(max_scratch_bytes) // (4 * n_c * max(n_slots, 1))
        if users < 1:
            raise CarcaHipError(f"{what}: one user's [C, n_slots] = [{n_c}, {n_slots}] fp32 logits need "
                                f"{4 * n_c * max(n_slots, 1)} bytes, max_scratch_bytes is {int(max_scratch_bytes)}")
        outs = _outputs(D, "ids_out", (D.B, n_c, k), dev)
        lib, stream = _lib.load(), ops._stream()
        for lo in range(0, D.B, users):
            Dc, Xc = _user_rows(D, X, lo, min(D.B, lo + users))
            if cand is None:
                rc = lib.carca_recommend_at(C.byref(Dc), C.byref(Xc), stream)
            else:
                rc = lib.carca_recommend_among_at(C.byref(Dc), C.byref(Xc), C.byref(cand), stream)
            _lib.check(rc, what)
        return outs


# ---- which profile slots drive a score (include/carca_hip.h: carca_explain_lists) --------------
EXPLAIN_TOP_MAX = 8  # largest m of explain_top_slots (csrc: EX_TOP_MAX, the insertion list a lane keeps in registers)


def _explain_m(what: str, m: int) -> int:
    if not 1 <= int(m) <= EXPLAIN_TOP_MAX:
        raise CarcaHipError(f"{what}: m = {m} outside 1..{EXPLAIN_TOP_MAX} (the most slots an explanation keeps is "
                            f"{EXPLAIN_TOP_MAX})")
    return int(m)


def _explain_launch(what: str, E, lst: Tensor, m: Optional[int], device) -> tuple:
    """Points E at the list and at fresh outputs and queues carca_explain_lists: m None -> the dense form,
    (scores, base, contrib [B, N, L], weights [B, H, N, L]); else the top-m form, (scores, base, slots, slot_items,
    contrib), each [B, N, m]."""
    B, N = E.B, lst.shape[1]
    _set_list(E, lst)
    scores = torch.empty(B, N, dtype=torch.float32, device=device)
    base = torch.empty(B, N, dtype=torch.float32, device=device)
    E.scores, E.ld_scores, E.base, E.ld_base = scores.data_ptr(), N, base.data_ptr(), N
    if m is None:
        contrib = torch.empty(B, N, E.L, dtype=torch.float32, device=device)
        weights = torch.empty(B, E.H, N, E.L, dtype=torch.float32, device=device)
        E.contrib, E.ld_contrib, E.weights, E.ld_weights = contrib.data_ptr(), E.L, weights.data_ptr(), E.L
        outs = (scores, base, contrib, weights)
    else:
        slots = torch.empty(B, N, m, dtype=torch.int64, device=device)
        slot_items = torch.empty(B, N, m, dtype=torch.int64, device=device)
        contrib = torch.empty(B, N, m, dtype=torch.float32, device=device)
        E.slots, E.ld_slots, E.slot_items, E.ld_slot_items = slots.data_ptr(), m, slot_items.data_ptr(), m
        E.contrib, E.ld_contrib, E.top_m = contrib.data_ptr(), m, m
        outs = (scores, base, slots, slot_items, contrib)
    _lib.check(_lib.load().carca_explain_lists(C.byref(E), ops._stream()), what)
    return outs


def explain_items(what: str, model_side: Callable, profile, items: Tensor) -> tuple:
    """The dense explanation of each user's own list: (scores [B, N], base [B, N], contrib [B, N, L],
    weights [B, H, N, L]), all float32."""
    with torch.no_grad():
        E, side, lst = _lists(what, model_side, profile, items, desc=_lib.ExplainDesc)
        return _explain_launch(what, E, lst, None, profile[0].device)


def explain_top_slots(what: str, model_side: Callable, profile, items: Tensor, m: int) -> tuple:
    """The m profile slots with the largest contribution per (user, list entry): (scores [B, N], base [B, N],
    slots [B, N, m] int64, slot_items [B, N, m] int64, contrib [B, N, m] float32); no [B, N, L] buffer."""
    m = _explain_m(what, m)
    with torch.no_grad():
        E, side, lst = _lists(what, model_side, profile, items, desc=_lib.ExplainDesc)
        return _explain_launch(what, E, lst, m, profile[0].device)


def recommend_explained(what: str, model_side: Callable, profile, k: int, m: int, exclude, candidates=None) -> tuple:
    """recommend, then explain_top_slots over its ids, with ONE run of the model side: one ModelSide fills the recommend
    descriptor and the explain descriptor.  -> (scores [B, k], ids [B, k], slot_items [B, k, m], contrib [B, k, m])."""
    _check_k(what, k)
    m = _explain_m(what, m)
    with torch.no_grad():
        side = model_side()
        D, keep = _topk_desc(what, side, k, exclude)
        device = profile[0].device
        cand = _candidates(what, candidates, D, keep, device)
        scores, ids = _launch(what, D, "carca_recommend", "ids_out", D.k, device, cand)
        E = side.desc(_lib.ExplainDesc)
        _, _, _, slot_items, contrib = _explain_launch(what, E, ops._ids32(ids), m, device)  # (id 0: no item)
        return scores, ids, slot_items, contrib


# ---- the k best users per listed item (include/carca_hip.h: carca_recommend_users) --------------
AUDIENCE_ID_END = 1 << 31  # user ids stay below it: the low word of a key holds the complemented id


class AudienceTopK:
    """The running k best users of each of Q listed items, over as many user batches as the caller feeds: the state behind
    CARCA.recommend_users and train.audience.

    items: a CandidateSet built for n_items, or a 1-D integer tensor / bool mask [n_items], normalised here (one host
    sync).  `ids` holds the item ids, int32 [Q], ascending and distinct: row q of the state and of every result belongs
    to item ids[q].  `keys` is the state, int64 [Q, k] holding unsigned 64-bit keys: the high word is the logit's
    order-preserving bits (csrc: rc::order_bits), the low word 0xFFFFFFFF minus the user id, 0 means empty, and every row is
    sorted descending (as unsigned) after every update.  A larger key is a larger logit and, between equal logits, the
    smaller user id; keys are distinct per user, so the state after a set of updates is the same bits however the users
    were split into updates and in whatever order the updates arrived.  Feeding one user id twice is the caller's error:
    both entries count.  `rows_seen` counts the rows of every update so far."""

    def __init__(self, items, k: int, n_items: int, device=None):
        what = "AudienceTopK"
        _check_k(what, k)
        if isinstance(items, CandidateSet):
            if items.n_items != int(n_items):
                raise CarcaHipError(f"{what}: the item set was built for n_items = {items.n_items}, the model has "
                                    f"{int(n_items)}")
        elif isinstance(items, Tensor):
            items = CandidateSet(items, n_items, device=device)
        else:
            raise CarcaHipError(f"{what}: items must be a CandidateSet or a 1-D integer / bool tensor")
        if device is not None:
            items = items.to(device)
        self.items, self.ids, self.k, self.n_items = items, items.ids, int(k), int(n_items)
        self.keys = torch.zeros(len(items), self.k, dtype=torch.int64, device=self.ids.device)
        self.rows_seen = 0
        self._decoder = None  # the link result() applies: the decoder code of the model that fed the state

    def reset(self) -> None:
        """Clears the state: no user seen, every entry empty (no host sync)."""
        self.keys.zero_()
        self.rows_seen = 0
        self._decoder = None

    def update(self, model, profile, context: Optional[Tensor], user_ids: Optional[Tensor] = None, exclude="profile",
               allow_composed: bool = False, _what: str = "AudienceTopK.update") -> None:
        """Merges one batch of users into the state: no host sync, nothing returned.  profile, context, exclude and
        allow_composed are CARCA.recommend's (user u is not eligible for an item its exclusion row lists).  user_ids: an
        int32 / int64 [B] tensor of ids below 2^31, a negative entry dropping its row; None numbers the rows from
        rows_seen on."""
        what = _what
        if not hasattr(model, "_check_eval_built") or not hasattr(model, "_catalogue_size"):
            raise CarcaHipError(f"{what}: model must be a CARCA ({type(model).__name__} has no users-per-item call)")
        model._check_eval_built(what)
        B, Q = profile[0].shape[0], len(self.items)
        n_known = model._catalogue_size()
        if n_known is not None and n_known != self.n_items:
            raise CarcaHipError(f"{what}: the item set was built for n_items = {self.n_items}, the model has {n_known}")
        if user_ids is not None:
            if not isinstance(user_ids, Tensor) or user_ids.dtype not in (torch.int32, torch.int64) or \
                    tuple(user_ids.shape) != (B,):
                raise CarcaHipError(f"{what}: user_ids must be an int32 / int64 [B = {B}] tensor")
        elif self.rows_seen + B >= AUDIENCE_ID_END:
            raise CarcaHipError(f"{what}: {self.rows_seen} rows seen + {B}: a row id would reach 2^31 (pass user_ids)")
        if B * Q >= 1 << 31:
            raise CarcaHipError(f"{what}: B * Q = {B * Q} does not fit an int (split the users)")
        with torch.no_grad():
            side = carca_model_side(model, profile, context, what, allow_composed)
            if side.fields["n_items"] != self.n_items:
                raise CarcaHipError(f"{what}: the item set was built for n_items = {self.n_items}, the model has "
                                    f"{side.fields['n_items']}")
            if self._decoder not in (None, side.fields["decoder"]):
                raise CarcaHipError(f"{what}: the state was fed by a model with another decoder (reset() it first)")
            D, keep = _topk_desc(what, side, self.k, exclude)
            ids = self.ids
            if ids.device != profile[0].device or self.keys.device != ids.device:
                raise CarcaHipError(f"{what}: the state lives on {ids.device}, the batch on {profile[0].device}")
            ops._need_cuda(ids, self.keys)
            cand = _lib.Candidates(ids.data_ptr() if Q else None, Q)
            state = _lib.Audience(self.keys.data_ptr() if Q else None, self.k, None, self.rows_seen)
            if user_ids is not None:
                ops._need_cuda(user_ids)
                # (clamped before the cast: no int64 id below -2^31 wraps into a user)
                u32 = ops._ids32(user_ids if user_ids.dtype == torch.int32 else user_ids.clamp(min=-1))
                keep.append(u32)
                state.user_ids, state.user_base = u32.data_ptr(), 0
            _lib.check(_lib.load().carca_recommend_users(C.byref(D), C.byref(cand), C.byref(state), ops._stream()), what)
            self._decoder = D.decoder
        self.rows_seen += B

    def result(self) -> Tuple[Tensor, Tensor, Tensor]:
        """(scores [Q, k] float32, users [Q, k] int64, item_ids [Q] int64): row q the k best eligible users seen so far for
        item item_ids[q], best first -- larger logit first, ties to the smaller user id; scores[q, j] is recommend's score
        of (users[q, j], item_ids[q]), bit for bit; fewer than k eligible users pad with user -1 and score 0.  The state
        is left as it is (no host sync)."""
        Q, k = self.keys.shape
        scores = torch.empty(Q, k, dtype=torch.float32, device=self.keys.device)
        users = torch.empty(Q, k, dtype=torch.int64, device=self.keys.device)
        if Q:
            ops._need_cuda(self.keys)
            rc = _lib.load().carca_audience_read(self.keys.data_ptr(), k, Q, k, self._decoder or 0, scores.data_ptr(),
                                                 users.data_ptr(), ops._stream())
            _lib.check(rc, "AudienceTopK.result")
        return scores, users, self.ids.to(torch.int64)


def recommend_users(model, profile, context: Optional[Tensor], items, k: int, exclude, user_ids: Optional[Tensor],
                    allow_composed: bool = False) -> Tuple[Tensor, Tensor, Tensor]:
    """CARCA.recommend_users: a fresh AudienceTopK on the batch's device, one update, result()."""
    n_items = model._catalogue_size()
    if n_items is None:  # (no id table and no registered attribute table to read it from: the cached item table's rows)
        with torch.no_grad():
            n_items = model.embeds.item_table().shape[0]
    state = AudienceTopK(items, k, n_items, device=profile[0].device)
    state.update(model, profile, context, user_ids, exclude, allow_composed, _what="recommend_users")
    return state.result()


# ---- item-to-item top-k (include/carca_hip.h: carca_similar_items) ------------------------------
SIMILAR_METRICS = {"dot": 0, "cosine": 1}  # CARCA_SIMILAR_DOT, CARCA_SIMILAR_COSINE
SIMILAR_BLOCK = 64  # queries per scoring workgroup (csrc: rs::QB): the granule of a chunk


def similar_chunk_rows(max_scratch_bytes: int, n_columns: int) -> int:
    """Queries per chunk: as many whole 64-query blocks as keep the [Qc, C] fp32 score buffer within max_scratch_bytes,
    and one block where the budget does not hold even that."""
    return max(SIMILAR_BLOCK, int(max_scratch_bytes) // (4 * max(int(n_columns), 1)) // SIMILAR_BLOCK * SIMILAR_BLOCK)


def similar_chunks(n_queries: int, chunk_rows: int) -> list:
    """The [start, stop) query slices of the chunk loop."""
    return [(s, min(n_queries, s + chunk_rows)) for s in range(0, n_queries, chunk_rows)]


def similar_args(what: str, items: Optional[Tensor], k: int, metric: str) -> None:
    """The argument checks that need no table."""
    _check_k(what, k)
    if metric not in SIMILAR_METRICS:
        raise ValueError(f'{what}: metric must be "cosine" or "dot", got {metric!r}')
    if items is not None and (not isinstance(items, Tensor) or items.dim() != 1 or items.is_floating_point()
                              or items.is_complex() or items.dtype == torch.bool):
        raise CarcaHipError(f"{what}: items must be None (every item) or a 1-D integer tensor of item ids")


def row_rnorm(table: Tensor, n_cols: int) -> Tensor:
    """r [n_rows] = 1 / max(||table[i, :n_cols]||, 1e-12) in fp32 (carca_row_rnorm)."""
    ops._need_cuda(table)
    out = torch.empty(table.shape[0], dtype=torch.float32, device=table.device)
    if table.shape[0]:
        _lib.check(_lib.load().carca_row_rnorm(table.data_ptr(), table.stride(0), table.shape[0], int(n_cols),
                                               out.data_ptr(), ops._stream()), "row_rnorm")
    return out


def similar_items(what: str, table: Tensor, n_cols: int, rnorm: Callable[[], Tensor], items: Optional[Tensor], k: int,
                  metric: str, exclude_self: bool, candidates=None, max_scratch_bytes: int = 1 << 30) -> Tuple[Tensor, Tensor]:
    """The k rows of `table` [n_items, ld] (fp32, n_cols live columns, ld a multiple of 4, 16-byte aligned) closest to each
    row listed in items: (scores [Q, k] float32, ids [Q, k] int64).  rnorm() gives the reciprocal row norms (row_rnorm of
    the table; called for "cosine" only, so a caller can cache them).  The queries go in chunks of similar_chunk_rows
    with no sync between them, each writing its slice of the outputs."""
    similar_args(what, items, k, metric)
    if isinstance(candidates, CandidateSet) and candidates.n_items != table.shape[0]:
        raise CarcaHipError(f"{what}: the candidate set was built for n_items = {candidates.n_items}, the table has "
                            f"{table.shape[0]}")
    ops._need_cuda(table, items)
    if table.dim() != 2 or table.dtype != torch.float32 or table.stride(1) != 1 or table.stride(0) % 4 or \
            table.data_ptr() % 16 or not 1 <= int(n_cols) <= table.shape[1]:
        raise CarcaHipError(f"{what}: the table must be float32 [n_items, >= n_cols] with unit column stride, a row stride "
                            "that is a multiple of 4 floats and a 16-byte aligned base")
    n_items, k, dev = table.shape[0], int(k), table.device
    with torch.no_grad():
        ids = torch.arange(n_items, dtype=torch.int32, device=dev) if items is None else _ids32_clamped(items, n_items)
        Q = ids.shape[0]
        D = _lib.SimilarDesc()
        D.n_items, D.n_cols, D.k = n_items, int(n_cols), k
        D.metric, D.exclude_self = SIMILAR_METRICS[metric], int(bool(exclude_self))
        keep = [table, ids]
        cand = _candidates(what, candidates, D, keep, dev)
        n_columns = n_items if cand is None else cand.n
        if Q == 0 or n_columns == 0:  # nothing to score: all padding, no launch
            return (torch.zeros(Q, k, dtype=torch.float32, device=dev), torch.zeros(Q, k, dtype=torch.int64, device=dev))
        scores = torch.empty(Q, k, dtype=torch.float32, device=dev)
        out_ids = torch.empty(Q, k, dtype=torch.int64, device=dev)
        D.table, D.ld_table = table.data_ptr(), table.stride(0)
        if metric == "cosine":
            rn = rnorm()
            keep.append(rn)
            D.rnorm = rn.data_ptr()
        if cand is not None:  # the listed rows (and their r), compacted by the first chunk's gather launch
            ldc = (int(n_cols) + 3) // 4 * 4
            ct = torch.empty(n_columns, ldc, dtype=torch.float32, device=dev)
            keep.append(ct)
            D.cand_table, D.ld_cand_table = ct.data_ptr(), ldc
            if metric == "cosine":
                cr = torch.empty(n_columns, dtype=torch.float32, device=dev)
                keep.append(cr)
                D.cand_rnorm = cr.data_ptr()
        D.ld_scores = D.ld_ids_out = k
        lib, stream = _lib.load(), ops._stream()
        for n, (lo, hi) in enumerate(similar_chunks(Q, similar_chunk_rows(max_scratch_bytes, n_columns))):
            D.Q, D.gather_candidates = hi - lo, int(n == 0)
            D.items = ids.data_ptr() + 4 * lo
            D.scores, D.ids_out = scores.data_ptr() + 4 * k * lo, out_ids.data_ptr() + 8 * k * lo
            _lib.check(lib.carca_similar_items(C.byref(D), None if cand is None else C.byref(cand), stream), what)
        return scores, out_ids


# ---- diversity re-ranking of a pool (include/carca_hip.h: carca_mmr_rerank) ---------------------
MMR_MAX_USERS = 65535  # users per launch (one workgroup each)


def mmr_args(what: str, k: int, pool: int, lam: float, metric: str) -> None:
    """The argument checks that need no tensor."""
    if metric not in SIMILAR_METRICS:
        raise ValueError(f'{what}: metric must be "cosine" or "dot", got {metric!r}')
    if not 0.0 <= float(lam) <= 1.0:  # (a NaN fails both comparisons)
        raise ValueError(f"{what}: lam = {lam} outside [0, 1]")
    if not 1 <= int(pool) <= KMAX:
        raise CarcaHipError(f"{what}: pool size {pool} outside 1..{KMAX} (the largest k recommend keeps is {KMAX})")
    if not 1 <= int(k) <= int(pool):
        raise CarcaHipError(f"{what}: k = {k} outside 1..pool = {pool}")


def mmr_rerank(what: str, scores: Tensor, ids: Tensor, table: Tensor, n_cols: int, k: int, lam: float, metric: str,
               normalize: bool, rnorm: Optional[Callable[[], Tensor]]) -> Tuple[Tensor, Tensor, Tensor]:
    """Greedy maximal-marginal-relevance re-rank of a pool (scores [B, P] float32, ids [B, P] integer, in pool order) over
    the rows of `table` [n_items, >= n_cols] (similar_items' layout rules): (scores [B, k] float32, ids [B, k] int64 in
    selection order, ild [B] float32).  rnorm() gives the table's reciprocal row norms (called for "cosine" only)."""
    if not isinstance(scores, Tensor) or not isinstance(ids, Tensor) or scores.dim() != 2 or ids.dim() != 2 or \
            tuple(scores.shape) != tuple(ids.shape):
        raise CarcaHipError(f"{what}: the pool must be scores [B, P] and ids [B, P] of one shape")
    if scores.dtype != torch.float32 or ids.is_floating_point() or ids.is_complex() or ids.dtype == torch.bool:
        raise CarcaHipError(f"{what}: pool scores must be float32 and pool ids an integer tensor, got {scores.dtype} and "
                            f"{ids.dtype}")
    B, P = scores.shape
    mmr_args(what, k, P, lam, metric)
    if not isinstance(table, Tensor) or table.dim() != 2 or table.dtype != torch.float32 or \
            not 1 <= int(n_cols) <= table.shape[1]:
        raise CarcaHipError(f"{what}: the table must be float32 [n_items, >= n_cols]")
    ops._need_cuda(scores, ids, table)
    if table.stride(1) != 1 or table.stride(0) % 4 or table.data_ptr() % 16:
        raise CarcaHipError(f"{what}: the table needs unit column stride, a row stride that is a multiple of 4 floats and a "
                            "16-byte aligned base")
    k, dev = int(k), table.device
    with torch.no_grad():
        out_s = torch.empty(B, k, dtype=torch.float32, device=dev)
        out_i = torch.empty(B, k, dtype=torch.int64, device=dev)
        ild = torch.empty(B, dtype=torch.float32, device=dev)
        if B == 0:
            return out_s, out_i, ild
        s = scores.detach() if scores.stride(1) == 1 else scores.detach().contiguous()
        i = ids.to(torch.int64)
        i = i if i.stride(1) == 1 else i.contiguous()
        D = _lib.MmrDesc()
        D.P, D.k, D.n_items, D.n_cols = P, k, table.shape[0], int(n_cols)
        D.metric, D.normalize, D.lam = SIMILAR_METRICS[metric], int(bool(normalize)), float(lam)
        D.table, D.ld_table = table.data_ptr(), table.stride(0)
        keep = [s, i, table]
        if metric == "cosine":
            rn = rnorm() if rnorm is not None else row_rnorm(table, n_cols)
            ops._need_cuda(rn)
            if rn.dtype != torch.float32 or rn.dim() != 1 or rn.shape[0] != table.shape[0] or not rn.is_contiguous():
                raise CarcaHipError(f"{what}: rnorm must be a contiguous float32 [n_items] tensor (catalogue.row_rnorm)")
            keep.append(rn)
            D.rnorm = rn.data_ptr()
        D.ld_pool_scores, D.ld_pool_ids, D.ld_scores, D.ld_ids_out = s.stride(0), i.stride(0), k, k
        lib, stream = _lib.load(), ops._stream()
        for lo in range(0, B, MMR_MAX_USERS):
            D.B = min(B - lo, MMR_MAX_USERS)
            D.pool_scores, D.pool_ids = s.data_ptr() + 4 * s.stride(0) * lo, i.data_ptr() + 8 * i.stride(0) * lo
            D.scores, D.ids_out, D.ild = out_s.data_ptr() + 4 * k * lo, out_i.data_ptr() + 8 * k * lo, ild.data_ptr() + 4 * lo
            _lib.check(lib.carca_mmr_rerank(C.byref(D), stream), what)
        return out_s, out_i, ild
