"""Full-catalogue softmax cross-entropy for the dot decoders (CARCA.catalogue_softmax_loss).

In train mode DotProduct / WeightedDotProduct pair profile slot t with target t (carca.py:358-367, 377-397):
z[b, t, i] = p[b, t] . e(i, c[b, t]).  Every embedding is affine in the context, e(i, c) = T[i] + M c, so the context's
share p . M c is the same for every item of the row and cancels in the softmax:

    CE = sum over valid r of ( logsumexp_{i = 1 .. n_items-1} P[r] . T[i] - P[r] . T[pos_r] ) / n_valid

with P the final-normed profile rows (times sum_{j<=t} gamma^j for WeightedDotProduct) and T the embedding of one target
segment arange(n_items) with zero context -- item_table(), but differentiable and not cached.  The loss runs in the fused
kernels of csrc/catalogue_xent.hip (ops.catalogue_xent_fwd / _bwd); its dP goes back through the decoder's slot weights,
the final LayerNorm and the encoder, its dT through the embedding's backward like any target segment's d e.

Profile side: the dot-decoder branch of autograd._CarcaFn (embed -> dropout -> sa_block_fwd(save=True) -> LayerNorm ->
slot decay) where the fused per-user kernels are built for the model; long_profile.py's differentiable pieces where
ops.use_composed says so."""
from __future__ import annotations

import torch
from torch import Tensor

from . import ops
from ._lib import CarcaHipError


def _check(model, profile, pos, what: str = "catalogue_softmax_loss") -> None:
    from .modules import CrossAttentionBlock, DotProduct, WeightedDotProduct, _need_attr_table

    dec, emb = model.decoder, model.embeds
    if isinstance(dec, CrossAttentionBlock):
        raise CarcaHipError(f"{what}: the CrossAttentionBlock decoder is not covered (the dot decoders "
                            "DotProduct / WeightedDotProduct(normalize=False) are)")
    if not isinstance(dec, (DotProduct, WeightedDotProduct)):
        raise CarcaHipError(f"{what}: decoder {type(dec).__name__} is not covered")
    if isinstance(dec, WeightedDotProduct) and dec.norm:
        raise CarcaHipError(f"{what}: WeightedDotProduct(normalize=True) divides by ||T[i] + M c||, which "
                            "depends on the context: the full-catalogue softmax does not reduce to the item table")
    model._check_built()
    p_x = profile[0]
    ops._need_cuda(p_x, profile[1], profile[2], pos)
    if tuple(pos.shape) != tuple(p_x.shape):
        raise CarcaHipError(f"{what}: pos must have the shape of p_x {tuple(p_x.shape)}, got "
                            f"{tuple(pos.shape)}")
    if hasattr(emb, "attr_table"):
        _need_attr_table(emb, what)
    if any(t is not None and t.requires_grad for t in profile):
        raise CarcaHipError("gradients with respect to the input tensors (ids/attrs/ctx) are not produced")


def _segments(model, profile):
    """[(profile segment), (catalogue segment: ids arange(n_items), attributes from the registered table, zero context)]."""
    emb = model.embeds
    p_x, p_a, p_c = profile
    n_items = emb.items_embed.num_embeddings if hasattr(emb, "items_embed") else emb.attr_table().shape[0]
    dev = p_x.device
    x = torch.arange(n_items, dtype=torch.int32, device=dev).view(1, n_items)
    c = torch.zeros(1, n_items, p_c.shape[-1], dtype=torch.float32, device=dev)
    c_ = lambda t: t if t.is_contiguous() else t.contiguous()  # noqa: E731
    cat_a = None  # AllEmbedding gathers the table's rows by id inside its products, forward and backward
    table = emb.attr_table() if hasattr(emb, "attr_table") else None
    if table is not None and not hasattr(emb, "items_embed"):
        # AttrCtx / Attr: their weight gradient reads dense attribute rows (modules._FeatsEmbedding.embed_backward)
        cat_a = table.view(1, n_items, table.shape[1])
        if p_a is None:
            p_a = table[p_x.long()]
    return [(c_(p_x), p_a, p_c, False), (x, cat_a, c, True)], n_items


def _profile_forward(model, segs):
    """The dot-decoder branch of autograd._CarcaFn over segs (the profile first, then target segments): the embedding of
    every segment, dropout, the encoder blocks (saved for the backward), the final LayerNorm and the slot decay.
    Returns (the final profile rows [B L, dpi], the embedded target segments, the state the backward reads)."""
    from .modules import WeightedDotProduct

    emb, dec = model.embeds, model.decoder
    d = emb.d
    dpi, _, _ = ops.padded_dims(d, model._heads())
    p_x = segs[0][0]
    B, L = p_x.shape
    if emb.__dict__.get("_fold_train"):  # CARCA.fold_embedding(True, training=True)
        es, emb_saved = emb._embed_segments_folded(segs, ld_e=dpi), "folded"
    else:
        es, emb_saved = emb.embed_segments(segs, ld_e=dpi)
    x = es[0]
    seed = ops.new_dropout_seed() if model.training else 0
    p_emb = float(model.dropout.p) if model.training else 0.0
    m_embed = ops.dropout_fwd(x, d, p_emb, seed, 1000) if p_emb > 0 else None  # carca.py:416
    repack: list = []
    sws = [blk.weights_struct(x.device, repack) for blk in model.encoder]
    ops.pack_many(repack)
    blocks = []
    for i, blk in enumerate(model.encoder):
        blk._check_mode()
        bp = blk.drop_p()
        y, saved = ops.sa_block_fwd(x, p_x, sws[i], d, blk.attn.H, blk.residual, save=True,
                                    drop=(bp, seed, 4 * i) if bp > 0 else None)
        saved["x_in"] = x
        saved["p"] = bp
        blocks.append(saved)
        x = y
    p_n = ops.layernorm_fwd(x.view(B * L, -1), model.norm.weight, model.norm.bias, d, dpi)  # carca.py:421
    rows = ops.slot_decay_scale(p_n, B, L, d, dec.gamma, dpi) if isinstance(dec, WeightedDotProduct) else p_n
    if getattr(model, "_keep_dropout_masks", False):  # test hook: the fused path's layout (autograd._CarcaFn)
        model._last_dropout_masks = dict(embed=m_embed, blocks=[{k: v for k, v in b.items() if k.startswith("m_")}
                                                                for b in blocks], cross=None)
    st = dict(p_x=p_x, segs=segs, es=es, emb_saved=emb_saved, blocks=blocks, enc_out=x, training=model.training,
              B=B, L=L, m_embed=m_embed, p_emb=p_emb, dpi=dpi, is_ca=False, rows=rows)
    return rows, es[1:], st


def _profile_backward(model, params, st, loss_bwd) -> tuple:
    """_profile_forward's backward -> the gradient of every parameter, as autograd._CarcaFn.backward computes it.
    loss_bwd() runs the loss's backward once the pass is set up and returns (dP [B L, dpi] of the final profile rows,
    [d e of every target segment, [rows, dpi] each])."""
    from .autograd import _encoder_backward, _prepare_backward
    from .modules import WeightedDotProduct

    emb, dec = model.embeds, model.decoder
    d, dpi, B, L = emb.d, st["dpi"], st["B"], st["L"]
    prep = _prepare_backward(model, params, st)
    plan, bpks, emb_wt_idx = prep["plan"], prep["bpks"], prep["emb_wt_idx"]
    grads, after_pass, det, gbp = prep["grads"], prep["after_pass"], prep["det"], prep["gbp"]
    dP, d_targets = loss_bwd()
    if isinstance(dec, WeightedDotProduct):  # the slot weights are diagonal: their own transpose
        dP = ops.slot_decay_scale(dP, B, L, d, dec.gamma, dpi)
    dx = ops.layernorm_bwd(dP, st["enc_out"].view(-1, dpi), model.norm.weight.detach(), d, dpi,
                           dgamma=gbp[id(model.norm.weight)], dbeta=gbp[id(model.norm.bias)])
    wg = ops.WgradGroup()
    dx = _encoder_backward(model, st, dx, gbp, bpks, wg)
    if st["p_emb"] > 0:  # CARCA.dropout on the profile embedding (carca.py:416)
        dx = ops.mask_mul(dx, st["m_embed"], 1.0 / (1.0 - st["p_emb"]), d, dpi)
    wg.launch()
    if det is not None:
        det.flush_staging()
    plan.unpack(gbp)
    des = [dx] + list(d_targets)
    if emb_wt_idx is not None:
        emb.embed_backward(des, st["segs"], st["emb_saved"], gbp, L, dpi, wj_t=plan.wT.view(emb_wt_idx))
    else:
        emb.embed_backward(des, st["segs"], st["emb_saved"], gbp, L, dpi)
    if det is not None:
        det.finish()
    after_pass()
    return tuple(grads)


class _CatalogueFn(torch.autograd.Function):
    """The fused route: one forward over the profile and the catalogue segment, one backward of fixed launches."""

    @staticmethod
    def forward(ctx, model, profile, pos, *params):
        segs, n_items = _segments(model, profile)
        rows, (cat,), st = _profile_forward(model, segs)
        T = cat.view(n_items, st["dpi"])
        pos32 = ops._ids32(pos.reshape(-1))
        loss, lse = ops.catalogue_xent_fwd(rows, T, pos32, model.embeds.d)
        ctx.model, ctx.params = model, params
        ctx.st = dict(st, T=T, pos=pos32, lse=lse)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        st, d = ctx.st, ctx.model.embeds.d

        def loss_bwd():
            dP, dT = ops.catalogue_xent_bwd(st["rows"], st["T"], st["pos"], st["lse"], g.detach(), d)
            return dP, [dT]

        grads = _profile_backward(ctx.model, ctx.params, st, loss_bwd)
        ctx.st = None
        return (None, None, None) + grads


def _composed_rows(model, profile, segs, what: str):
    """long_profile.py's differentiable pieces (L > 64, d > 128 or an unbuilt (d, H)) over segs, the profile first:
    (the normalised profile rows [B, L, d] with the decoder's weights, the target segments' embeddings)."""
    from . import long_profile as lp
    from .modules import WeightedDotProduct, cached_parameters

    emb, dec = model.embeds, model.decoder
    L = profile[0].shape[1]
    if L > 1024:
        raise CarcaHipError(f"{what}: L={L} > 1024 profile slots")
    training = model.training
    seed = ops.new_dropout_seed() if training else 0
    sink = lp._Sink(len(model.encoder), 0) if getattr(model, "_keep_dropout_masks", False) else None
    x, *targets = lp._EmbedSegsFn.apply(emb, tuple(segs), *cached_parameters(emb))
    if training and model.dropout.p > 0:  # carca.py:416
        x = lp._DropoutFn.apply(x, float(model.dropout.p), seed, 1000, sink, ("embed",))
    for i, blk in enumerate(model.encoder):
        blk._check_mode()
        x = lp.sa_block(blk, x, segs[0][0], seed, 4 * i, sink, i)
    p_n = lp._norm(x, model.norm)  # carca.py:421
    if isinstance(dec, WeightedDotProduct):  # p[t] * sum_{j<=t} gamma^j (carca.py:385-386)
        w = torch.cumsum(dec.gamma ** torch.arange(L, dtype=torch.float64, device=p_n.device), 0).to(torch.float32)
        p_n = p_n * w.view(1, L, 1)
    if sink is not None:
        model._last_dropout_masks = sink.masks
    return p_n, targets


def _composed_loss(model, profile, pos) -> Tensor:
    segs, n_items = _segments(model, profile)
    p_n, (T,) = _composed_rows(model, profile, segs, "catalogue_softmax_loss")
    d = model.embeds.d
    return ops.catalogue_xent(p_n.reshape(-1, d), T.reshape(n_items, d), pos.reshape(-1))


def catalogue_softmax_loss(model, profile, pos: Tensor) -> Tensor:
    from .modules import cached_parameters, note_training_forward

    _check(model, profile, pos)
    note_training_forward()  # packed-weight caches: see modules._WEIGHT_EPOCH
    if model._composed(profile, [profile]):
        return _composed_loss(model, profile, pos)
    return _CatalogueFn.apply(model, tuple(profile), pos, *cached_parameters(model))


# ---- the policy's log-probabilities, differentiable ----------------------------------------------
def profile_exclusion(p_x: Tensor) -> Tensor:
    """exclude="profile" for every slot: [B, L, L] with row (b, t) holding p_x[b, :t + 1] and 0 (padding) after it -- at
    t = L - 1 recommend(exclude="profile")'s rule.  Torch ops on p_x's device, no host wait."""
    L = p_x.shape[1]
    keep = torch.ones(L, L, dtype=torch.bool, device=p_x.device).tril()
    return torch.where(keep.unsqueeze(0), p_x.unsqueeze(1), torch.zeros((), dtype=p_x.dtype, device=p_x.device))


def _policy_args(model, profile, items, temperature, exclude, what: str, last_only: bool = False):
    """The checks of log_prob_rows' own arguments -> (items [B L] int32 with the rows of padding slots set to 0, the
    temperature as fp32, the sorted exclusion lists [B L, E] int32 or None); with last_only the rows of slot L - 1 alone
    ([B] and [B, E]; "profile" is then p_x itself, one list per user)."""
    p_x = profile[0]
    if not isinstance(items, Tensor) or tuple(items.shape) != tuple(p_x.shape) or items.is_floating_point() or \
            items.dtype == torch.bool:
        raise CarcaHipError(f"{what}: items must be an int tensor of p_x's shape {tuple(p_x.shape)}, got "
                            f"{tuple(items.shape) if isinstance(items, Tensor) else type(items).__name__}")
    t32 = ops.policy_temperature(what, temperature)
    _check(model, profile, items, what)
    emb = model.embeds
    n_items = emb.items_embed.num_embeddings if hasattr(emb, "items_embed") else emb.attr_table().shape[0]
    B, L = p_x.shape
    if exclude is None:
        excl = None
    elif isinstance(exclude, str):
        if exclude != "profile":
            raise CarcaHipError(f'{what}: exclude must be None, "profile" or an int [B, L, E] tensor, got {exclude!r}')
        excl = p_x.reshape(B, 1, L) if last_only else profile_exclusion(p_x)
    else:
        if not isinstance(exclude, Tensor) or exclude.dim() != 3 or tuple(exclude.shape[:2]) != (B, L) or \
                exclude.is_floating_point() or exclude.dtype == torch.bool:
            raise CarcaHipError(f'{what}: exclude must be None, "profile" or an int [B, L, E] tensor with B, L = {B}, {L}')
        ops._need_cuda(exclude)
        excl = exclude[:, L - 1:] if last_only else exclude
    live = torch.where(p_x != 0, items, torch.zeros_like(items))
    if last_only:
        live = live[:, L - 1]
    R = live.numel()
    excl_sorted = ops.policy_exclusion(excl.reshape(R, -1), R, n_items) if excl is not None else None
    return ops._ids32_clamped(live.reshape(-1), n_items), t32, excl_sorted


def _last_slot(full_shape, last: Tensor) -> Tensor:
    """[B] values of slot L - 1 -> [B, L] with zeros (False) elsewhere."""
    out = torch.zeros(full_shape, dtype=last.dtype, device=last.device)
    out[:, -1] = last
    return out


class _PolicyRowsFn(torch.autograd.Function):
    """_CatalogueFn with ops.policy_xent_fwd / _bwd: per-row outputs, per-row upstream gradients.  last_only: the op runs
    over the B rows of slot L - 1 alone (a contiguous copy of them), the other rows are not valid by construction."""

    @staticmethod
    def forward(ctx, model, profile, items32, t32, excl_sorted, with_entropy, last_only, *params):
        segs, n_items = _segments(model, profile)
        rows, (cat,), st = _profile_forward(model, segs)
        B, L, dpi = st["B"], st["L"], st["dpi"]
        T = cat.view(n_items, dpi)
        P = rows.view(B, L, dpi)[:, L - 1].contiguous() if last_only else rows
        log_prob, valid, entropy, lse = ops.policy_xent_fwd(P, T, items32, model.embeds.d, t32, excl_sorted, with_entropy)
        ctx.model, ctx.params = model, params
        ctx.st = dict(st, T=T, px=(P, items32, t32, excl_sorted, lse, valid, entropy, last_only))
        full = (lambda t: _last_slot((B, L), t)) if last_only else (lambda t: t.view(B, L))
        out = (full(log_prob), full(valid))
        ctx.mark_non_differentiable(out[1])
        return out + (full(entropy),) if with_entropy else out

    @staticmethod
    def backward(ctx, g_lp, g_valid, g_ent=None):
        st, d = ctx.st, ctx.model.embeds.d
        P, items32, t32, excl_sorted, lse, valid, entropy, last_only = st["px"]
        B, L, dpi = st["B"], st["L"], st["dpi"]
        rows_of = (lambda g: g.detach()[:, L - 1].contiguous()) if last_only else (lambda g: g.detach().reshape(-1))

        def loss_bwd():
            c = rows_of(g_lp) if g_lp is not None else torch.zeros_like(lse)
            h = None
            if entropy is not None:
                h = rows_of(g_ent) if g_ent is not None else torch.zeros_like(lse)
            dP, dT = ops.policy_xent_bwd(P, st["T"], items32, d, t32, excl_sorted, lse, c, h, entropy, valid)
            if last_only:
                dP_last, dP = dP, torch.zeros(B, L, dpi, dtype=torch.float32, device=dP.device)
                dP[:, L - 1] = dP_last
                dP = dP.view(B * L, dpi)
            return dP, [dT]

        grads = _profile_backward(ctx.model, ctx.params, st, loss_bwd)
        ctx.st = None
        return (None,) * 7 + grads


def log_prob_rows(model, profile, items: Tensor, temperature: float = 1.0, exclude=None, with_entropy: bool = False,
                  last_slot_only: bool = False):
    from .modules import cached_parameters, note_training_forward

    what = "log_prob_rows"
    last = bool(last_slot_only)
    items32, t32, excl_sorted = _policy_args(model, profile, items, temperature, exclude, what, last)
    note_training_forward()  # packed-weight caches: see modules._WEIGHT_EPOCH
    B, L = profile[0].shape
    if model._composed(profile, [profile]):
        segs, n_items = _segments(model, profile)
        p_n, (T,) = _composed_rows(model, profile, segs, what)
        d = model.embeds.d
        P = p_n[:, L - 1] if last else p_n.reshape(-1, d)
        out = ops._PolicyXentFn.apply(P, T.reshape(n_items, d), items32, t32, excl_sorted, bool(with_entropy))
        out = tuple(_last_slot((B, L), o) if last else o.view(B, L) for o in out)
    else:
        out = _PolicyRowsFn.apply(model, tuple(profile), items32, t32, excl_sorted, bool(with_entropy), last,
                                  *cached_parameters(model))
    return (out[0], out[1], out[2]) if with_entropy else (out[0], out[1], None)


# ---- sampled softmax with the logQ correction ------------------------------------------------
def _sampled_segments(model, profile, pos, samples):
    """[(profile segment), (samples [1, K], zero context), (positives [B, L], zero context)]; sample and positive ids
    outside [1, n_items) become 0 on the device (the embedding's padding row, never a class)."""
    emb = model.embeds
    p_x, p_a, p_c = profile
    n_items = emb.items_embed.num_embeddings if hasattr(emb, "items_embed") else emb.attr_table().shape[0]
    dev = p_x.device

    def fix(ids):
        ids = ids.to(torch.int32)
        return torch.where((ids >= 1) & (ids < n_items), ids, torch.zeros_like(ids))

    s = fix(samples.reshape(1, -1))
    tp = fix(pos)
    K = s.shape[1]
    c_s = torch.zeros(1, K, p_c.shape[-1], dtype=torch.float32, device=dev)
    c_p = torch.zeros(*tp.shape, p_c.shape[-1], dtype=torch.float32, device=dev)
    c_ = lambda t: t if t.is_contiguous() else t.contiguous()  # noqa: E731
    a_s = a_p = None  # AllEmbedding gathers the table's rows by id inside its products, forward and backward
    table = emb.attr_table() if hasattr(emb, "attr_table") else None
    if table is not None and not hasattr(emb, "items_embed"):
        # AttrCtx / Attr: their weight gradient reads dense attribute rows (modules._FeatsEmbedding.embed_backward)
        a_s, a_p = table[s.long()], table[tp.long()]
        if p_a is None:
            p_a = table[p_x.long()]
    return [(c_(p_x), p_a, p_c, False), (s, a_s, c_s, True), (tp, a_p, c_p, True)], n_items


class _SampledFn(torch.autograd.Function):
    """The fused route of the sampled loss: _CatalogueFn's, with the samples and the positives as the target segments."""

    @staticmethod
    def forward(ctx, model, profile, pos, samples, log_q, *params):
        segs, n_items = _sampled_segments(model, profile, pos, samples)
        rows, (es_s, es_p), st = _profile_forward(model, segs)
        dpi, K = st["dpi"], segs[1][0].shape[1]
        S, Tp = es_s.view(K, dpi), es_p.view(-1, dpi)
        pos32, s32, bp, bs = ops.sampled_xent_corrections(pos, samples, log_q)
        d = model.embeds.d
        loss, lse, row_loss = ops.sampled_xent_fwd(rows, Tp, bp, pos32, S, s32, bs, n_items, d)
        ctx.model, ctx.params = model, params
        ctx.st = dict(st, S=S, Tp=Tp, sx=(bp, pos32, s32, bs, n_items), lse=lse, row_loss=row_loss)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        st, d = ctx.st, ctx.model.embeds.d

        def loss_bwd():
            bp, pos32, s32, bs, n_items = st["sx"]
            dP, dTp, dS = ops.sampled_xent_bwd(st["rows"], st["Tp"], bp, pos32, st["S"], s32, bs, n_items, st["lse"],
                                               st["row_loss"], g.detach(), d)
            return dP, [dS, dTp]

        grads = _profile_backward(ctx.model, ctx.params, st, loss_bwd)
        ctx.st = None
        return (None, None, None, None, None) + grads


def _sampled_composed_loss(model, profile, pos, samples, log_q) -> Tensor:
    segs, _ = _sampled_segments(model, profile, pos, samples)
    p_n, (S, Tp) = _composed_rows(model, profile, segs, "sampled_softmax_loss")
    d = model.embeds.d
    return ops.sampled_xent(p_n.reshape(-1, d), Tp.reshape(-1, d), pos.reshape(-1), S.reshape(-1, d),
                            samples.reshape(-1), log_q)


def sampled_softmax_loss(model, profile, pos: Tensor, samples: Tensor, log_q: Tensor) -> Tensor:
    from .modules import cached_parameters, note_training_forward

    what = "sampled_softmax_loss"
    _check(model, profile, pos, what)
    ops._need_cuda(samples, log_q)
    if samples.is_floating_point() or samples.numel() < 1:
        raise CarcaHipError(f"{what}: samples must be a non-empty integer tensor of item ids")
    emb = model.embeds
    n_items = emb.items_embed.num_embeddings if hasattr(emb, "items_embed") else emb.attr_table().shape[0]
    if log_q.dim() != 1 or log_q.numel() != n_items or not log_q.is_floating_point():
        raise CarcaHipError(f"{what}: log_q must be a float tensor [n_items = {n_items}], got {tuple(log_q.shape)} "
                            f"{log_q.dtype}")
    note_training_forward()  # packed-weight caches: see modules._WEIGHT_EPOCH
    if model._composed(profile, [profile]):
        return _sampled_composed_loss(model, profile, pos, samples, log_q)
    return _SampledFn.apply(model, tuple(profile), pos, samples, log_q, *cached_parameters(model))


# ---- softmax over per-user negative lists ------------------------------------------------------
def _listed_operands(negatives):
    """(the ids of the [1, U] target segment, the CSR for them): NegativeLists' own, or, for an all-padding object, one
    padding id (a segment needs a row; no entry points to it) with the CSR of that one row."""
    if len(negatives) > 0:
        return negatives.ids, (negatives.csr_off, negatives.csr_ent)
    return torch.zeros(1, dtype=torch.int32, device=negatives.ids.device), ops.listed_csr(negatives.index, 1)


class _ListedFn(torch.autograd.Function):
    """The fused route of the listed loss: _SampledFn's, with the lists' distinct items as the [1, U] target segment."""

    @staticmethod
    def forward(ctx, model, profile, pos, negatives, *params):
        ids, csr = _listed_operands(negatives)
        segs, n_items = _sampled_segments(model, profile, pos, ids)
        rows, (es_s, es_p), st = _profile_forward(model, segs)
        dpi, U, L = st["dpi"], segs[1][0].shape[1], st["L"]
        S, Tp = es_s.view(U, dpi), es_p.view(-1, dpi)
        pos32 = ops._ids32_clamped(pos.reshape(-1), n_items)
        d = model.embeds.d
        lx = (pos32, negatives.lists, negatives.index, L, negatives.bias, None, n_items)
        loss, lse, row_loss = ops.listed_xent_fwd(rows, Tp, pos32, S, negatives.lists, negatives.index, L, negatives.bias,
                                                  None, n_items, d)
        ctx.model, ctx.params = model, params
        ctx.st = dict(st, S=S, Tp=Tp, lx=lx, csr=csr, lse=lse, row_loss=row_loss)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        st, d = ctx.st, ctx.model.embeds.d

        def loss_bwd():
            pos32, lists, index, L, bias, pos_bias, n_items = st["lx"]
            dP, dTp, dS = ops.listed_xent_bwd(st["rows"], st["Tp"], pos32, st["S"], lists, index, L, bias, pos_bias,
                                              n_items, st["csr"], st["lse"], st["row_loss"], g.detach(), d)
            return dP, [dS, dTp]

        grads = _profile_backward(ctx.model, ctx.params, st, loss_bwd)
        ctx.st = None
        return (None, None, None, None) + grads


def _listed_composed_loss(model, profile, pos, negatives) -> Tensor:
    ids, csr = _listed_operands(negatives)
    segs, n_items = _sampled_segments(model, profile, pos, ids)
    p_n, (S, Tp) = _composed_rows(model, profile, segs, "listed_softmax_loss")
    d, L = model.embeds.d, profile[0].shape[1]
    return ops.listed_xent(p_n.reshape(-1, d), Tp.reshape(-1, d), pos.reshape(-1), S.reshape(-1, d), negatives.lists,
                           negatives.index, L, negatives.bias, n_items=n_items, csr=csr)


def listed_softmax_loss(model, profile, pos: Tensor, negatives) -> Tensor:
    from .catalogue import NegativeLists
    from .modules import cached_parameters, note_training_forward

    what = "listed_softmax_loss"
    _check(model, profile, pos, what)
    emb = model.embeds
    n_items = emb.items_embed.num_embeddings if hasattr(emb, "items_embed") else emb.attr_table().shape[0]
    B, L = profile[0].shape
    if not isinstance(negatives, NegativeLists):
        if not isinstance(negatives, Tensor):
            raise CarcaHipError(f"{what}: negatives must be a NegativeLists or an integer tensor [B, N]")
        ops._need_cuda(negatives)
        negatives = NegativeLists(negatives, n_items)
    if negatives.n_items != n_items:
        raise CarcaHipError(f"{what}: the negative lists were built for n_items = {negatives.n_items}, the model has "
                            f"{n_items}")
    if negatives.G != B:
        raise CarcaHipError(f"{what}: one list per user is needed, [B = {B}, N]; got {negatives.G} lists")
    if L > ops.LISTED_MAX_ROWS_PER_LIST:
        raise CarcaHipError(f"{what}: L={L} > {ops.LISTED_MAX_ROWS_PER_LIST} profile slots")
    negatives = negatives.to(profile[0].device)
    ops._need_cuda(negatives.ids)
    note_training_forward()  # packed-weight caches: see modules._WEIGHT_EPOCH
    if model._composed(profile, [profile]):
        return _listed_composed_loss(model, profile, pos, negatives)
    return _ListedFn.apply(model, tuple(profile), pos, negatives, *cached_parameters(model))


# ---- BCE against K shared negatives, gBCE ------------------------------------------------------
def _context_rows(model, pos_ctx: Tensor):
    """C [B L, d] = M c_r, the context's share of e(i, c) = T[i] + M c, as a differentiable function of the embedding's
    weights (M = W_jq W_f[:, n_attrs:] for AllEmbedding, W_j W_f[:, n_attrs:] for AttrCtxEmbedding), so that the loss's dC
    reaches them: two row products of autograd._LinearFn, c W_f,ctx^T then W_jq^T, without the biases (they are T's).
    None for an embedding without a context term.  (Not context_matrix(): that one is cached and detached.)"""
    from .autograd import _LinearFn
    from .modules import AllEmbedding, _FeatsEmbedding

    emb = model.embeds
    n_ctx = pos_ctx.shape[-1]
    if n_ctx == 0:
        return None
    if isinstance(emb, AllEmbedding):
        w_jq = emb.joint_embed.weight[:, emb.d:]
    elif isinstance(emb, _FeatsEmbedding) and emb._use_ctx:
        w_jq = emb.joint_embed.weight
    else:
        return None
    w_f = emb.feats_embed.weight
    g, F = w_f.shape
    # the context block of W_f and the context rows, zero-padded to a multiple of 4 columns (the row product's 16-byte
    # operand rows); the pad is differentiable, so dW_f lands in the block's columns
    pad = -n_ctx % 4
    w_c = torch.nn.functional.pad(w_f[:, F - n_ctx:], (0, pad))
    c = torch.nn.functional.pad(pos_ctx.reshape(-1, n_ctx).to(torch.float32), (0, pad))
    zero = lambda n: torch.zeros(n, dtype=torch.float32, device=c.device)  # noqa: E731
    q = _LinearFn.apply(c, w_c, zero(g))
    return _LinearFn.apply(q, w_jq, zero(emb.d))


def _bce_segments(model, profile, pos, pos_ctx, samples):
    """_sampled_segments with the positives' own context: [(profile), (samples [1, K], zero context), (positives [B, L],
    pos_ctx)]."""
    segs, n_items = _sampled_segments(model, profile, pos, samples)
    tp, a_p, _, tgt = segs[2]
    segs[2] = (tp, a_p, pos_ctx.to(torch.float32).contiguous(), tgt)
    return segs, n_items


class _SampledBceFn(torch.autograd.Function):
    """The fused route of the gBCE loss: _SampledFn's, with the rows' context share C as one more differentiable input."""

    @staticmethod
    def forward(ctx, model, profile, pos, pos_ctx, samples, beta, Cr, *params):
        segs, n_items = _bce_segments(model, profile, pos, pos_ctx, samples)
        rows, (es_s, es_p), st = _profile_forward(model, segs)
        dpi, K = st["dpi"], segs[1][0].shape[1]
        S, Tp = es_s.view(K, dpi), es_p.view(-1, dpi)
        pos32, s32 = ops._ids32(pos.reshape(-1)), ops._ids32(samples.reshape(-1))
        d = model.embeds.d
        C2 = ops._xent_operand(Cr.detach(), d, "sampled_bce_loss") if Cr is not None else None
        loss, saved, _ = ops.sampled_bce_fwd(rows, Tp, C2, pos32, S, s32, n_items, beta, d)
        ctx.model, ctx.params = model, params
        ctx.st = dict(st, S=S, Tp=Tp, C=C2, sb=(pos32, s32, n_items, beta), saved=saved)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        st, d = ctx.st, ctx.model.embeds.d
        out = {}

        def loss_bwd():
            pos32, s32, n_items, beta = st["sb"]
            dP, dTp, dS, dC = ops.sampled_bce_bwd(st["rows"], st["Tp"], st["C"], pos32, st["S"], s32, n_items, beta,
                                                  st["saved"], g.detach(), d)
            out["dC"] = dC
            return dP, [dS, dTp]

        grads = _profile_backward(ctx.model, ctx.params, st, loss_bwd)
        ctx.st = None
        dC = out["dC"][:, :d] if out["dC"] is not None else None
        return (None, None, None, None, None, None, dC) + grads


def _bce_composed_loss(model, profile, pos, pos_ctx, samples, beta, Cr) -> Tensor:
    segs, n_items = _bce_segments(model, profile, pos, pos_ctx, samples)
    p_n, (S, Tp) = _composed_rows(model, profile, segs, "sampled_bce_loss")
    d = model.embeds.d
    return ops.sampled_bce(p_n.reshape(-1, d), Tp.reshape(-1, d), pos.reshape(-1), S.reshape(-1, d), samples.reshape(-1),
                           n_items, beta, C=Cr)


def sampled_bce_loss(model, profile, pos: Tensor, pos_ctx: Tensor, samples: Tensor, t: float = 0.75) -> Tensor:
    from .modules import cached_parameters, note_training_forward

    what = "sampled_bce_loss"
    _check(model, profile, pos, what)
    ops._need_cuda(samples, pos_ctx)
    if samples.is_floating_point() or samples.numel() < 1:
        raise CarcaHipError(f"{what}: samples must be a non-empty integer tensor of item ids")
    p_c = profile[2]
    if pos_ctx.dim() != 3 or tuple(pos_ctx.shape[:2]) != tuple(pos.shape) or pos_ctx.shape[2] != p_c.shape[-1]:
        raise CarcaHipError(f"{what}: pos_ctx must be [B, L, n_ctx] = {tuple(pos.shape) + (p_c.shape[-1],)}, got "
                            f"{tuple(pos_ctx.shape)}")
    if pos_ctx.requires_grad:
        raise CarcaHipError("gradients with respect to the input tensors (ids/attrs/ctx) are not produced")
    emb = model.embeds
    n_items = emb.items_embed.num_embeddings if hasattr(emb, "items_embed") else emb.attr_table().shape[0]
    beta = ops.sampled_bce_beta(samples.numel(), n_items, t)  # (t outside [0, 1]: ValueError)
    note_training_forward()  # packed-weight caches: see modules._WEIGHT_EPOCH
    Cr = _context_rows(model, pos_ctx)
    if model._composed(profile, [profile]):
        return _bce_composed_loss(model, profile, pos, pos_ctx, samples, beta, Cr)
    return _SampledBceFn.apply(model, tuple(profile), pos, pos_ctx, samples, beta, Cr, *cached_parameters(model))
