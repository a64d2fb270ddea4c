"""Build and load libcarca_hip.so (the C ABI declared in include/carca_hip.h) with ctypes.

The library is built IN-TREE (``carca_replication_amd/libcarca_hip.so``) by ``build()`` with
``hipcc --offload-arch=gfx950``; the built file travels to the GPU box with the repo snapshot.
There is no CPU fallback: if the library cannot be built or loaded, every op raises.
"""
from __future__ import annotations

import ctypes as C
import hashlib
import os
import shutil
import subprocess
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
_INCLUDE = os.path.join(os.path.dirname(_HERE), "include")
LIB_PATH = os.path.join(_HERE, "libcarca_hip.so")
_STAMP = LIB_PATH + ".srchash"
SOURCES = ["api.hip", "gemm.hip", "gemm_wgrad.hip", "gemm_split.hip", "gemm_stream.hip", "wgrad_cu.hip", "decoders.hip", "batch_build.hip", "embed.hip", "sa_block.hip", "sa_eval.hip", "cross_score.hip", "cross_stream.hip", "loss_metrics.hip", "backward.hip", "block_bwd.hip", "row_chain.hip", "optim.hip", "recommend.hip", "rank.hip", "knn_catalogue.hip",
           "catalogue_xent.hip", "feat_dedup.hip", "sampled_xent.hip", "sampled_bce.hip", "similar_items.hip", "mmr_rerank.hip", "recommend_lists.hip", "explain_lists.hip",
           "recommend_users.hip", "recommend_contexts.hip", "retrieve.hip", "recommend_sampled.hip", "policy_items.hip", "policy_xent.hip", "listed_xent.hip"]
HEADERS = ["carca_common.h", "gemm_host.h", "attn_common.h", "gemm_epilogue.h", "gemm_tile384.h", "cross_fold.h", "recommend_common.h", "catalogue_select.h",
           "catalogue_sweep.h", "xent_tile.h", "xent_stage.h", "xent_direct.h", "row_stream.h", "group_select.h", "recommend_score.h", "deep_select.h",
           "sampled_select.h", "policy_items.h"]

MAX_SEGS = 4
MAX_GROUPS = 3
MAX_L = 64
MAX_PROFILE_L = 1024  # CARCA_MAX_PROFILE_L: profile slots of carca_recommend / carca_rank_items

_lock = threading.Lock()
_lib = None


class CarcaHipError(RuntimeError):
    pass


def _source_hash() -> str:
    h = hashlib.sha256()
    for name in SOURCES + HEADERS:
        p = os.path.join(_CSRC, name)
        if os.path.exists(p):
            with open(p, "rb") as f:
                h.update(name.encode() + b"\0" + f.read())
    with open(os.path.join(_INCLUDE, "carca_hip.h"), "rb") as f:
        h.update(f.read())
    return h.hexdigest()


def _hipcc() -> str | None:
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


def is_built() -> bool:
    if not os.path.exists(LIB_PATH) or not os.path.exists(_STAMP):
        return False
    with open(_STAMP) as f:
        return f.read().strip() == _source_hash()


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile every HIP source for gfx950 into one shared library (cross-compiles without a GPU)."""
    import fcntl

    # one builder at a time ACROSS processes too (torchrun ranks, pytest workers on a fresh checkout): the objects go to
    # fixed paths under build/, and a rank that links another rank's half-written object gets a corrupt library
    with _lock, open(os.path.join(_HERE, ".build.lock"), "w") as lockf:
        fcntl.flock(lockf, fcntl.LOCK_EX)
        if not force and is_built():  # (re-checked under the lock: another process may just have finished)
            return LIB_PATH
        hipcc = _hipcc()
        if hipcc is None:
            raise CarcaHipError("hipcc not found: cannot build libcarca_hip.so (no CPU fallback exists)")
        srcs = [os.path.join(_CSRC, s) for s in SOURCES if os.path.exists(os.path.join(_CSRC, s))]
        objs = []
        procs = []
        os.makedirs(os.path.join(_HERE, "build"), exist_ok=True)
        for s in srcs:
            o = os.path.join(_HERE, "build", os.path.basename(s) + ".o")
            objs.append(o)
            cmd = [hipcc, "-O3", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-c", s, "-o", o]
            procs.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
        for cmd, p in procs:
            out, _ = p.communicate()
            if p.returncode != 0:
                raise CarcaHipError("hipcc failed: " + " ".join(cmd) + "\n" + out)
            if verbose and out.strip():
                print(out)
        tmp = LIB_PATH + ".tmp"
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", tmp] + objs
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise CarcaHipError("link failed: " + " ".join(cmd) + "\n" + r.stdout)
        os.replace(tmp, LIB_PATH)
        with open(_STAMP, "w") as f:
            f.write(_source_hash())
        global _lib
        _lib = None
        return LIB_PATH


# ---- ctypes mirrors of the structs in include/carca_hip.h ------------------------------------------
_fp = C.c_void_p  # device pointers travel as integers


class PackDesc(C.Structure):
    _fields_ = [("src", _fp), ("dst", _fp), ("rows", C.c_int32), ("cols", C.c_int32), ("src_ld", C.c_int32),
                ("dst_rows", C.c_int32), ("dst_cols", C.c_int32), ("row_dh", C.c_int32), ("row_dhp", C.c_int32),
                ("col_dh", C.c_int32), ("col_dhp", C.c_int32), ("transposed", C.c_int32), ("frag16", C.c_int32),
                ("fold_vec", _fp), ("fold_H", C.c_int32)]


class RowSeg(C.Structure):
    _fields_ = [("ids", _fp), ("attrs", _fp), ("ctx", _fp), ("e_out", _fp), ("rows", C.c_int32), ("T", C.c_int32),
                ("add_pos", C.c_int32), ("attrs_bstride", C.c_int64), ("ctx_bstride", C.c_int64),
                ("attrs_table", _fp), ("attrs_table_rows", C.c_int32)]


class GemmSeg(C.Structure):
    _fields_ = [("a0", _fp), ("a1", _fp), ("c", _fp), ("ids", _fp), ("add", _fp), ("gate", _fp), ("rowscale", _fp),
                ("rows", C.c_int32), ("T", C.c_int32), ("add_pos", C.c_int32), ("a0_bstride", C.c_int64),
                ("a1_bstride", C.c_int64), ("a0_gather", C.c_int32)]


class GemmDesc(C.Structure):
    _fields_ = [("seg", GemmSeg * MAX_SEGS), ("nseg", C.c_int32), ("lda0", C.c_int32), ("lda1", C.c_int32),
                ("K0", C.c_int32), ("K1", C.c_int32), ("bt0", _fp), ("bt1", _fp), ("ldb0", C.c_int32),
                ("ldb1", C.c_int32), ("N", C.c_int32), ("ldc", C.c_int32), ("ncols_out", C.c_int32), ("bias", _fp),
                ("pos", _fp), ("colvec", _fp), ("ld_add", C.c_int32), ("ld_gate", C.c_int32),
                ("gate_slope", C.c_float), ("mask_rows", C.c_int32), ("alpha", C.c_float), ("gate_scale", C.c_float),
                ("gate_zero_drops", C.c_int32), ("add_table", _fp), ("ld_add_table", C.c_int32)]


class WgradSeg(C.Structure):
    _fields_ = [("dy", _fp), ("x", _fp), ("x1", _fp), ("ids", _fp), ("rows", C.c_int32), ("T", C.c_int32),
                ("x_bstride", C.c_int64), ("x1_bstride", C.c_int64), ("x_gather", C.c_int32)]


class WgradDesc(C.Structure):
    _fields_ = [("seg", WgradSeg * MAX_SEGS), ("nseg", C.c_int32), ("ld_dy", C.c_int32), ("ld_x", C.c_int32),
                ("ld_x1", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("K1", C.c_int32), ("dw", _fp),
                ("ldw", C.c_int32), ("db", _fp), ("mask_rows", C.c_int32)]


class Dropout(C.Structure):
    _fields_ = [("p", C.c_float), ("seed", C.c_uint64), ("site", C.c_uint32), ("seed_offset", C.c_void_p)]


class SaSave(C.Structure):
    _fields_ = [(n, _fp) for n in ("qn", "qh", "kh", "vh", "r", "s2", "h1", "m_attn", "m_ffn1", "m_ffn2")]


class CaSave(C.Structure):
    _fields_ = [("kh", _fp), ("vh", _fp), ("qh", _fp * MAX_GROUPS), ("m_attn", _fp * MAX_GROUPS)]


class CrossBwdGroup(C.Structure):
    _fields_ = [("qh", _fp), ("y", _fp), ("dy", _fp), ("ids", _fp), ("dqh", _fp), ("dlogit", _fp), ("m_attn", _fp),
                ("N", C.c_int32), ("ld_y", C.c_int32)]


class AdamTensor(C.Structure):
    _fields_ = [("p", _fp), ("g", _fp), ("m", _fp), ("v", _fp), ("n", C.c_int64), ("row_mask", _fp), ("row_len", C.c_int64)]


class SaBwdDesc(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("B", "L", "d", "H", "residual")] + [("drop_p", C.c_float), ("ids", _fp), ("dy", _fp)]
                + [(n, _fp) for n in ("x_in", "qn", "qh", "kh", "vh", "r", "s2", "h1", "m_attn", "m_ffn2", "wq_t", "wk_t",
                                      "wv_t", "w1_t", "w2_t", "ln1_w", "ln2_w", "g_w1", "g_b1", "g_w2", "g_b2", "g_wq",
                                      "g_wk", "g_wv", "g_bq", "g_bk", "g_bv", "g_ln1_w", "g_ln1_b", "g_ln2_w", "g_ln2_b",
                                      "workspace", "dx")])


class CrossBwdIn(C.Structure):
    _fields_ = [(n, _fp) for n in ("qh", "y", "dy", "ids", "o", "m_attn", "de")] + [("N", C.c_int32), ("ld_y", C.c_int32)]


class CrossBwdDesc(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("B", "L", "d", "H", "ngroups", "residual", "training")] + [("drop_p", C.c_float),
                ("group", CrossBwdIn * MAX_GROUPS)]
                + [(n, _fp) for n in ("p_ids", "kh", "vh", "p_normed", "enc_out", "wq_t", "wk_t", "wv_t", "ffn_w_pad", "ffn_w",
                                      "norm_w", "g_ffn_w", "g_ffn_b", "g_ffn_w_pad", "g_wq", "g_wk", "g_wv", "g_bq", "g_bk",
                                      "g_bv", "g_norm_w", "g_norm_b", "workspace", "dx")])


class EmbedBwdSeg(C.Structure):
    _fields_ = [(n, _fp) for n in ("de", "ids", "attrs", "ctx", "attrs_table")] + [
        ("attrs_bstride", C.c_int64), ("ctx_bstride", C.c_int64), ("rows", C.c_int32), ("T", C.c_int32),
        ("attrs_table_rows", C.c_int32), ("joint_only", C.c_int32)]


class EmbedBwdDesc(C.Structure):
    _fields_ = ([("seg", EmbedBwdSeg * MAX_SEGS)] + [(n, C.c_int32) for n in ("nseg", "d", "g", "n_attrs", "n_ctx", "ld_de", "L")]
                + [("zq", _fp), ("joint_wt", _fp), ("ld_joint_wt", C.c_int32)]
                + [(n, _fp) for n in ("g_items", "g_feats_w", "g_feats_b", "g_joint_w", "g_joint_b", "g_pos", "workspace",
                                      "ev_early")] + [("skip_joint", C.c_int32)])


class SaWeights(C.Structure):
    _fields_ = [(n, _fp) for n in ("ln1_w", "ln1_b", "ln2_w", "ln2_b", "wq", "wk", "wv", "bq", "bk", "bv", "w1", "w2",
                                   "b1", "b2")]


class CaWeights(C.Structure):
    _fields_ = [(n, _fp) for n in ("ln_w", "ln_b", "wq", "wk", "wv", "bq", "bk", "bv", "ffn_w_pad", "ffn_w", "ffn_b", "wu", "cu")]


class TargetGroup(C.Structure):
    _fields_ = [("o", _fp), ("ids", _fp), ("y", _fp), ("N", C.c_int32), ("ldy", C.c_int32)]


MAX_BLOCKS = 8


class ForwardDesc(C.Structure):
    _fields_ = [("segs", RowSeg * MAX_SEGS), ("ngroups", C.c_int32), ("B", C.c_int32), ("L", C.c_int32),
                ("d", C.c_int32), ("g", C.c_int32), ("H", C.c_int32), ("n_attrs", C.c_int32), ("n_ctx", C.c_int32),
                ("n_blocks", C.c_int32), ("ld_e", C.c_int32), ("items_w", _fp), ("feats_w", _fp), ("feats_b", _fp),
                ("joint_w", _fp), ("joint_b", _fp), ("pos", _fp), ("zq", _fp), ("x_work", _fp * 2),
                ("sa", SaWeights * MAX_BLOCKS), ("sa_residual", C.c_int32 * MAX_BLOCKS), ("ca", CaWeights),
                ("ca_residual", C.c_int32), ("training", C.c_int32), ("y", _fp * MAX_GROUPS),
                ("N", C.c_int32 * MAX_GROUPS), ("ldy", C.c_int32), ("p_normed", _fp), ("fold_wc", _fp), ("fold_bias", _fp),
                ("fold_ldwc", C.c_int32), ("x_out", _fp * MAX_BLOCKS), ("sa_save", SaSave * MAX_BLOCKS), ("ca_save", CaSave),
                ("save_blocks", C.c_int32), ("save_cross", C.c_int32), ("p_embed", C.c_float), ("p_block", C.c_float),
                ("p_cross", C.c_float), ("seed", C.c_uint64), ("m_embed", _fp), ("seed_offset", C.c_void_p),
                ("n_events", C.c_int32), ("z_table", _fp), ("ld_z_table", C.c_int32)]


# name -> (restype, argtypes); every symbol include/carca_hip.h declares
_i, _f = C.c_int, C.c_float
# the model-side and exclusion fields of CarcaRecommendDesc / CarcaRankDesc, `decoder` through `ld_exclude`
_CARCA_MODEL = [("decoder", C.c_int32), ("p_ids", _fp), ("ld_p_ids", C.c_int32), ("item_q", _fp), ("ld_item_q", C.c_int32),
                ("item_w", _fp), ("ld_item_w", C.c_int32), ("user_k", _fp), ("ld_user_k", C.c_int32), ("user_u", _fp),
                ("ld_user_u", C.c_int32), ("user_q", _fp), ("ld_user_q", C.c_int32), ("user_m", _fp),
                ("ld_user_m", C.c_int32), ("user_off", _fp), ("ld_user_off", C.c_int32), ("ffn_b", _fp), ("exclude", _fp),
                ("n_exclude", C.c_int32), ("ld_exclude", C.c_int32)]
_TOPK_OUT = [("scores", _fp), ("ld_scores", C.c_int32), ("ids_out", _fp), ("ld_ids_out", C.c_int32)]
_RANK_OUT = [("items", _fp), ("n_list", C.c_int32), ("ld_items", C.c_int32), ("scores", _fp), ("ld_scores", C.c_int32),
             ("ranks", _fp), ("ld_ranks", C.c_int32)]


class RecommendDesc(C.Structure):
    """CarcaRecommendDesc (carca_recommend)."""
    _fields_ = [(n, C.c_int32) for n in ("B", "L", "n_items", "d", "H", "k")] + _CARCA_MODEL + _TOPK_OUT


class RankDesc(C.Structure):
    """CarcaRankDesc (carca_rank_items)."""
    _fields_ = [(n, C.c_int32) for n in ("B", "L", "n_items", "d", "H")] + _CARCA_MODEL + _RANK_OUT


class ListsDesc(C.Structure):
    """CarcaListsDesc (carca_score_lists / carca_recommend_lists)."""
    _fields_ = [(n, C.c_int32) for n in ("B", "L", "n_items", "d", "H", "k")] + _CARCA_MODEL + [
        ("items", _fp), ("n_list", C.c_int32), ("ld_items", C.c_int32), ("sorted_rows", C.c_int32)] + _TOPK_OUT


class ExplainDesc(C.Structure):
    """CarcaExplainDesc (carca_explain_lists)."""
    _fields_ = [(n, C.c_int32) for n in ("B", "L", "n_items", "d", "H", "k")] + _CARCA_MODEL + [
        ("items", _fp), ("n_list", C.c_int32), ("ld_items", C.c_int32), ("scores", _fp), ("ld_scores", C.c_int32),
        ("base", _fp), ("ld_base", C.c_int32), ("contrib", _fp), ("ld_contrib", C.c_int32), ("weights", _fp),
        ("ld_weights", C.c_int32), ("slots", _fp), ("ld_slots", C.c_int32), ("slot_items", _fp),
        ("ld_slot_items", C.c_int32), ("top_m", C.c_int32)]


class Candidates(C.Structure):
    """CarcaCandidates (carca_recommend_among / carca_rank_items_among)."""
    _fields_ = [("ids", _fp), ("n", C.c_int32)]


class Sampling(C.Structure):
    """CarcaSampling (carca_recommend_sampled / carca_knn_recommend_sampled)."""
    _fields_ = [("temperature", C.c_float), ("seed", C.c_uint64), ("user_keys", _fp), ("log_probs", _fp),
                ("ld_log_probs", C.c_int32)]


class Contexts(C.Structure):
    """CarcaContexts (carca_score_lists_at / carca_recommend_at / carca_recommend_among_at)."""
    _fields_ = [("n_contexts", C.c_int32), ("user_q", _fp), ("ld_user_q", C.c_int32), ("user_off", _fp),
                ("ld_user_off", C.c_int32), ("user_m", _fp), ("ld_user_m", C.c_int32)]


class ItemGroups(C.Structure):
    """CarcaItemGroups (carca_recommend_groups / carca_recommend_capped)."""
    _fields_ = [("order", _fp), ("offsets", _fp), ("pos_of", _fp), ("n", C.c_int32), ("n_groups", C.c_int32)]


class Audience(C.Structure):
    """CarcaAudience (carca_recommend_users)."""
    _fields_ = [("keys", _fp), ("ld_keys", C.c_int32), ("user_ids", _fp), ("user_base", C.c_int32)]


_KNN_MODEL = [("p_ids", _fp), ("ld_p_ids", C.c_int32), ("user_a", _fp), ("ld_user_a", C.c_int64), ("table", _fp),
              ("ld_table", C.c_int32), ("table_i8", _fp), ("ld_table_i8", C.c_int32), ("exclude", _fp),
              ("n_exclude", C.c_int32), ("ld_exclude", C.c_int32)]


class KnnRecommendDesc(C.Structure):
    """CarcaKnnRecommendDesc (carca_knn_recommend)."""
    _fields_ = [(n, C.c_int32) for n in ("B", "L", "n_items", "F", "k")] + _KNN_MODEL + _TOPK_OUT


class KnnRankDesc(C.Structure):
    """CarcaKnnRankDesc (carca_knn_rank_items)."""
    _fields_ = [(n, C.c_int32) for n in ("B", "L", "n_items", "F")] + _KNN_MODEL + _RANK_OUT

class CatalogueXentDesc(C.Structure):
    """CarcaCatalogueXentDesc (carca_catalogue_xent_fwd / _bwd)."""
    _fields_ = [("R", C.c_int32), ("n_items", C.c_int32), ("d", C.c_int32), ("P", _fp), ("ld_p", C.c_int32), ("T", _fp),
                ("ld_t", C.c_int32), ("pos", _fp), ("splits_items", C.c_int32), ("items_per_split", C.c_int32),
                ("splits_rows", C.c_int32), ("scratch", _fp), ("scratch_floats", C.c_int64), ("lse", _fp),
                ("row_loss", _fp), ("loss", _fp), ("grad", _fp), ("dP", _fp), ("dT", _fp)]


class PolicyXentDesc(C.Structure):
    """CarcaPolicyXentDesc (carca_policy_xent_fwd / _bwd)."""
    _fields_ = [("R", C.c_int32), ("n_items", C.c_int32), ("d", C.c_int32), ("P", _fp), ("ld_p", C.c_int32), ("T", _fp),
                ("ld_t", C.c_int32), ("items", _fp), ("temperature", C.c_float), ("excl", _fp), ("n_excl", C.c_int32),
                ("t_off", _fp), ("t_rows", _fp), ("splits_items", C.c_int32), ("items_per_split", C.c_int32),
                ("splits_rows", C.c_int32), ("scratch", _fp), ("scratch_floats", C.c_int64), ("lse", _fp),
                ("log_prob", _fp), ("entropy", _fp), ("valid", _fp), ("c", _fp), ("h", _fp), ("dP", _fp), ("dT", _fp)]


class PolicyItems(C.Structure):
    """CarcaPolicyItems (carca_log_prob_items / carca_knn_log_prob_items)."""
    _fields_ = [("temperature", C.c_float), ("items", _fp), ("n_list", C.c_int32), ("ld_items", C.c_int32),
                ("log_probs", _fp), ("ld_log_probs", C.c_int32), ("lse", _fp), ("entropy", _fp)]


class SampledXentDesc(C.Structure):
    """CarcaSampledXentDesc (carca_sampled_xent_fwd / _bwd)."""
    _fields_ = [("R", C.c_int32), ("K", C.c_int32), ("n_items", C.c_int32), ("d", C.c_int32), ("P", _fp),
                ("ld_p", C.c_int32), ("Tp", _fp), ("ld_tp", C.c_int32), ("bp", _fp), ("pos", _fp), ("S", _fp),
                ("ld_s", C.c_int32), ("s_ids", _fp), ("bs", _fp), ("splits_samples", C.c_int32),
                ("samples_per_split", C.c_int32), ("splits_rows", C.c_int32), ("scratch", _fp),
                ("scratch_floats", C.c_int64), ("lse", _fp), ("row_loss", _fp), ("loss", _fp), ("grad", _fp),
                ("dP", _fp), ("dTp", _fp), ("dS", _fp)]


class ListedXentDesc(C.Structure):
    """CarcaListedXentDesc (carca_listed_xent_fwd / _bwd)."""
    _fields_ = [(n, C.c_int32) for n in ("R", "G", "rows_per_list", "N", "U", "n_items", "d")] + [
        ("P", _fp), ("ld_p", C.c_int32), ("Tp", _fp), ("ld_tp", C.c_int32), ("pos_bias", _fp), ("pos", _fp), ("S", _fp),
        ("ld_s", C.c_int32), ("lists", _fp), ("index", _fp), ("bias", _fp), ("csr_off", _fp), ("csr_ent", _fp),
        ("splits", C.c_int32), ("entries_per_split", C.c_int32), ("scratch", _fp), ("scratch_floats", C.c_int64),
        ("lse", _fp), ("row_loss", _fp), ("loss", _fp), ("grad", _fp), ("dP", _fp), ("dTp", _fp), ("dS", _fp)]


class SampledBceDesc(C.Structure):
    """CarcaSampledBceDesc (carca_sampled_bce_fwd / _bwd)."""
    _fields_ = [("R", C.c_int32), ("K", C.c_int32), ("n_items", C.c_int32), ("d", C.c_int32), ("P", _fp),
                ("ld_p", C.c_int32), ("Tp", _fp), ("ld_tp", C.c_int32), ("C", _fp), ("ld_c", C.c_int32), ("pos", _fp),
                ("S", _fp), ("ld_s", C.c_int32), ("s_ids", _fp), ("beta", C.c_float), ("splits_samples", C.c_int32),
                ("samples_per_split", C.c_int32), ("splits_rows", C.c_int32), ("scratch", _fp),
                ("scratch_floats", C.c_int64), ("zpos", _fp), ("br", _fp), ("gsum", _fp), ("row_loss", _fp),
                ("loss", _fp), ("grad", _fp), ("dP", _fp), ("dTp", _fp), ("dC", _fp), ("dS", _fp)]


class SimilarDesc(C.Structure):
    """CarcaSimilarDesc (carca_similar_items)."""
    _fields_ = [(n, C.c_int32) for n in ("Q", "n_items", "n_cols", "k", "metric", "exclude_self")] + [
        ("table", _fp), ("ld_table", C.c_int32), ("rnorm", _fp), ("items", _fp), ("cand_table", _fp),
        ("ld_cand_table", C.c_int32), ("cand_rnorm", _fp), ("gather_candidates", C.c_int32)] + _TOPK_OUT


class MmrDesc(C.Structure):
    """CarcaMmrDesc (carca_mmr_rerank)."""
    _fields_ = [(n, C.c_int32) for n in ("B", "P", "k", "n_items", "n_cols", "metric", "normalize")] + [
        ("lam", C.c_float), ("pool_scores", _fp), ("ld_pool_scores", C.c_int32), ("pool_ids", _fp),
        ("ld_pool_ids", C.c_int32), ("table", _fp), ("ld_table", C.c_int32), ("rnorm", _fp)] + _TOPK_OUT + [("ild", _fp)]


class FeatCache(C.Structure):  # CarcaFeatCache
    _fields_ = [("p_c", _fp), ("a_c", _fp), ("state", _fp), ("table", _fp), ("n_rows", C.c_int32), ("ld_p", C.c_int32),
                ("ld_a", C.c_int32)]



SIGNATURES = {
    "carca_abi_version": (_i, []),
    "carca_set_tuning": (_i, [_i, _i]),
    "carca_det_begin": (_i, [_fp, C.c_longlong, _fp, _fp]),
    "carca_det_flush": (_i, [_fp, _fp, C.c_longlong, C.c_longlong, _fp]),
    "carca_set_debug_buffer": (_i, [_fp]),
    "carca_last_error": (C.c_char_p, []),
    "carca_poll_errors": (_i, []),
    "carca_capture_scope": (_i, [_fp, C.POINTER(C.c_ulonglong)]),
    "carca_capture_bytes": (C.c_longlong, [C.c_ulonglong]),
    "carca_capture_release": (_i, [C.c_ulonglong]),
    "carca_release_stream_scratch": (_i, [_fp]),
    "carca_padded_dims": (_i, [_i, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "carca_attn_geometry_built": (_i, [_i, _i]),
    "carca_pack_weights": (_i, [C.POINTER(PackDesc), _i, _fp]),
    "carca_embed_fwd": (_i, [C.POINTER(RowSeg), _i, _i, _i, _i, _i, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _i, _i, _fp]),
    "carca_gemm_rows": (_i, [C.POINTER(GemmDesc), _fp]),
    "carca_split_bytes": (C.c_longlong, [_i, _i, _i]),
    "carca_split_pack": (_i, [_fp, _i, _i, _i, _i, _fp, _fp]),
    "carca_split_bind": (_i, [_fp, _fp, _i, _i, _i]),
    "carca_split_launch_count": (C.c_longlong, []),
    "carca_gemm_rows_group": (_i, [C.POINTER(GemmDesc), _i, _fp]),
    "carca_gemm_wgrad": (_i, [C.POINTER(WgradDesc), _fp]),
    "carca_gemm_wgrad_group": (_i, [C.POINTER(WgradDesc), _i, _fp]),
    "carca_sa_block_fwd": (_i, [_fp, _i, _fp, _fp, _i, _i, _i, _i, _i, C.POINTER(SaWeights), _i, C.POINTER(SaSave),
                                C.POINTER(Dropout), _fp]),
    "carca_sa_block_eval": (_i, [_fp, _i, _fp, _fp, _i, _i, _i, _i, _i, C.POINTER(SaWeights), _i, _i, _fp]),
    "carca_cross_score_fwd": (_i, [_fp, _i, _fp, _fp, C.POINTER(TargetGroup), _i, _i, _i, _i, _i, _i,
                                   C.POINTER(CaWeights), _i, _i, C.POINTER(CaSave), C.POINTER(Dropout), _fp]),
    "carca_dropout_fwd": (_i, [_fp, _i, _i, _i, C.POINTER(Dropout), _fp, _fp]),
    "carca_mask_mul": (_i, [_fp, _i, _fp, _i, _f, _fp, _i, _i, _i, _i, _fp]),
    "carca_layernorm_bwd": (_i, [_fp, _i, _fp, _i, _fp, _i, _i, _fp, _i, _fp, _i, _i, _fp, _fp, _fp]),
    "carca_embed_scatter": (_i, [_fp, _i, _fp, _i, _i, _f, _fp, _fp]),
    "carca_colsum": (_i, [_fp, _i, _i, _i, _fp, _fp, _i, _fp, _fp]),
    "carca_sa_attn_bwd": (_i, [_fp, _fp, _fp, _fp, _i, _fp, _fp, _fp, _fp, _i, _i, _i, _i, _fp, _f, _fp]),
    "carca_cross_attn_bwd": (_i, [_fp, _fp, _fp, C.POINTER(CrossBwdGroup), _i, _fp, _fp, _fp, _fp, _i, _i, _i, _i, _i,
                                  _f, _fp]),
    "carca_unpack_grads": (_i, [C.POINTER(PackDesc), _i, _i, _fp]),
    "carca_forward": (_i, [C.POINTER(ForwardDesc), C.POINTER(_fp), _fp]),
    "carca_event_create": (_i, [C.POINTER(_fp)]),
    "carca_event_destroy": (_i, [_fp]),
    "carca_event_elapsed_ms": (_i, [_fp, _fp, C.POINTER(C.c_float)]),
    "carca_stream_wait_event": (_i, [_fp, _fp]),
    "carca_bce_fwd": (_i, [_fp, _fp, _fp, _i, _f, _fp, _fp, _fp, _fp, _fp]),
    "carca_rank_metrics": (_i, [_fp, _i, _i, _i, _fp, _fp, _fp, _fp]),
    "carca_eval_metrics": (_i, [_fp, _fp, _fp, _i, _i, _i, _f, _fp, _fp]),
    "carca_layernorm_fwd": (_i, [_fp, _i, _fp, _i, _i, _i, _fp, _fp, _fp]),
    "carca_dot_score_fwd": (_i, [_fp, _i, _fp, _i, _fp, _i, _i, _i, _i, _i, _i, _fp]),
    "carca_dot_score_bwd": (_i, [_fp, _i, _fp, _i, _fp, _fp, _fp, _i, _fp, _i, _i, _i, _i, _i, _i, _i, _fp]),
    "carca_slot_decay_scale": (_i, [_fp, _i, _fp, _i, _i, _i, _i, _f, _fp]),
    "carca_l2norm_fwd": (_i, [_fp, _i, _fp, _i, _i, _i, _fp]),
    "carca_l2norm_bwd": (_i, [_fp, _i, _fp, _i, _fp, _i, _i, _i, _fp]),
    "carca_add_positions": (_i, [_fp, _i, _fp, _fp, _i, _i, _i, _i, _fp]),
    "carca_mha_core": (_i, [_fp, _i, _fp, _fp, _i, _fp, _fp, _i, _i, _i, _i, _i, _i, _i, _fp, _i, _fp, _fp]),
    "carca_mha_core_bwd": (_i, [_fp, _i, _fp, _fp, _i, _fp, _fp, _i, _i, _i, _i, _i, _i, _i, _fp, _i, _fp, _fp, _fp, _fp,
                                _fp]),
    "carca_gemm_rows_log": (_i, [C.c_char_p, _i]),
    "carca_feat_dedup_rows_multiplied": (C.c_longlong, []),
    "carca_feat_dedup_rows_computed": (C.c_longlong, []),
    "carca_feat_dedup_rows_grouped": (C.c_longlong, []),
    "carca_sa_eval_lent": (C.c_longlong, []),
    "carca_feat_cache_arm": (_i, [C.POINTER(FeatCache)]),
    "carca_get_tuning": (_i, [_i]),
    "carca_mha_core_drop": (_i, [_fp, _i, _fp, _fp, _i, _fp, _fp, _i, _i, _i, _i, _i, _i, _i, _fp, _i, _fp, C.POINTER(Dropout),
                                 _fp, _fp]),
    "carca_mha_core_bwd_drop": (_i, [_fp, _i, _fp, _fp, _i, _fp, _fp, _i, _i, _i, _i, _i, _i, _i, _fp, _i, _fp, _fp, _fp, _fp,
                                     _fp, C.c_float, _fp]),
    "carca_knn_score": (_i, [_fp, C.c_int64, _fp, C.c_int64, _fp, _fp, _i, _fp, _i, _i, _i, _i, _fp]),
    "carca_sa_block_bwd_workspace": (C.c_size_t, [_i, _i, _i, _i]),
    "carca_sa_block_bwd": (_i, [C.POINTER(SaBwdDesc), C.POINTER(WgradDesc), C.POINTER(_i), _fp]),
    "carca_cross_score_bwd_workspace": (C.c_size_t, [_i, _i, _i, _i, C.POINTER(C.c_int32), _i]),
    "carca_cross_score_bwd": (_i, [C.POINTER(CrossBwdDesc), C.POINTER(WgradDesc), C.POINTER(_i), _fp]),
    "carca_embed_bwd_workspace": (C.c_size_t, [C.POINTER(C.c_int32), _i, _i, _i]),
    "carca_embed_bwd": (_i, [C.POINTER(EmbedBwdDesc), _fp]),
    "carca_early_event_recorded": (_i, []),
    "carca_adam_step": (_i, [C.POINTER(AdamTensor), _i, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, _i,
                        _fp]),
    "carca_adam_step_ex": (_i, [C.POINTER(AdamTensor), _i, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, _i,
                           _i, _fp, _fp]),
    "carca_grad_norm": (_i, [C.POINTER(AdamTensor), _i, C.c_double, _fp, C.c_int64, _fp, _fp]),
    "carca_mark_rows": (_i, [_fp, C.c_int64, _fp, C.c_int64, _fp]),
    "carca_zero_rows": (_i, [_fp, C.c_int64, _i, C.POINTER(_fp), C.POINTER(C.c_int64), _i, _fp]),
    "carca_concat_ids": (_i, [C.POINTER(_fp), C.POINTER(C.c_int64), _i, _fp, _fp]),
    "carca_build_eval_batch": (_i, [_fp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _i, _i, _i, C.c_uint64, _fp, _fp, _fp, _fp, _fp,
                                    _fp]),
    "carca_recommend": (_i, [C.POINTER(RecommendDesc), _fp]),
    "carca_rank_items": (_i, [C.POINTER(RankDesc), _fp]),
    "carca_recommend_among": (_i, [C.POINTER(RecommendDesc), C.POINTER(Candidates), _fp]),
    "carca_rank_items_among": (_i, [C.POINTER(RankDesc), C.POINTER(Candidates), _fp]),
    "carca_retrieve": (_i, [C.POINTER(RecommendDesc), _fp]),
    "carca_retrieve_among": (_i, [C.POINTER(RecommendDesc), C.POINTER(Candidates), _fp]),
    "carca_knn_retrieve": (_i, [C.POINTER(KnnRecommendDesc), _fp]),
    "carca_recommend_sampled": (_i, [C.POINTER(RecommendDesc), C.POINTER(Candidates), C.POINTER(Sampling), _fp]),
    "carca_sampled_perturb": (_i, [_fp, _fp, _fp, _i, _i, C.POINTER(Sampling), _fp]),
    "carca_knn_recommend_sampled": (_i, [C.POINTER(KnnRecommendDesc), C.POINTER(Candidates), C.POINTER(Sampling), _fp]),
    "carca_log_prob_items": (_i, [C.POINTER(RecommendDesc), C.POINTER(Candidates), C.POINTER(PolicyItems), _fp]),
    "carca_policy_reduce": (_i, [_fp, _fp, _i, _i, _f, _fp]),
    "carca_knn_log_prob_items": (_i, [C.POINTER(KnnRecommendDesc), C.POINTER(Candidates), C.POINTER(PolicyItems), _fp]),
    "carca_recommend_groups": (_i, [C.POINTER(RecommendDesc), C.POINTER(ItemGroups), _fp]),
    "carca_recommend_capped": (_i, [C.POINTER(RecommendDesc), C.POINTER(ItemGroups), _i, _fp]),
    "carca_recommend_users": (_i, [C.POINTER(RecommendDesc), C.POINTER(Candidates), C.POINTER(Audience), _fp]),
    "carca_audience_read": (_i, [_fp, _i, _i, _i, _i, _fp, _fp, _fp]),
    "carca_score_lists": (_i, [C.POINTER(ListsDesc), _fp]),
    "carca_recommend_lists": (_i, [C.POINTER(ListsDesc), _fp]),
    "carca_score_lists_at": (_i, [C.POINTER(ListsDesc), C.POINTER(Contexts), _fp, _i, _fp]),
    "carca_recommend_at": (_i, [C.POINTER(RecommendDesc), C.POINTER(Contexts), _fp]),
    "carca_recommend_among_at": (_i, [C.POINTER(RecommendDesc), C.POINTER(Contexts), C.POINTER(Candidates), _fp]),
    "carca_explain_lists": (_i, [C.POINTER(ExplainDesc), _fp]),
    "carca_knn_recommend": (_i, [C.POINTER(KnnRecommendDesc), _fp]),
    "carca_knn_rank_items": (_i, [C.POINTER(KnnRankDesc), _fp]),
    "carca_row_rnorm": (_i, [_fp, _i, _i, _i, _fp, _fp]),
    "carca_similar_items": (_i, [C.POINTER(SimilarDesc), C.POINTER(Candidates), _fp]),
    "carca_mmr_rerank": (_i, [C.POINTER(MmrDesc), _fp]),
    "carca_catalogue_xent_fwd": (_i, [C.POINTER(CatalogueXentDesc), _fp]),
    "carca_catalogue_xent_bwd": (_i, [C.POINTER(CatalogueXentDesc), _fp]),
    "carca_policy_xent_fwd": (_i, [C.POINTER(PolicyXentDesc), _fp]),
    "carca_policy_xent_bwd": (_i, [C.POINTER(PolicyXentDesc), _fp]),
    "carca_sampled_xent_fwd": (_i, [C.POINTER(SampledXentDesc), _fp]),
    "carca_sampled_xent_bwd": (_i, [C.POINTER(SampledXentDesc), _fp]),
    "carca_listed_xent_fwd": (_i, [C.POINTER(ListedXentDesc), _fp]),
    "carca_listed_xent_bwd": (_i, [C.POINTER(ListedXentDesc), _fp]),
    "carca_sampled_bce_fwd": (_i, [C.POINTER(SampledBceDesc), _fp]),
    "carca_sampled_bce_bwd": (_i, [C.POINTER(SampledBceDesc), _fp]),
    "carca_build_train_batch": (_i, [_fp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _i, _i, C.c_uint64, _fp, _fp, _fp, _fp, _fp,
                                     _fp]),
}


def declared_symbols() -> list[str]:
    """Function names declared in include/carca_hip.h (parsed from the header text)."""
    import re

    with open(os.path.join(_INCLUDE, "carca_hip.h")) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(carca_[a-z0-9_]+)\s*\(", text)))


def load():
    """Load the library (building it first if the sources changed) and type its entry points."""
    global _lib
    if _lib is not None:
        return _lib
    # torch must load ITS libamdhip64.so.7 first: the library below has the same soname, and a process
    # that resolves it to /opt/rocm's copy before torch starts ends up with a runtime that sees no device
    import torch  # noqa: F401

    if not is_built():
        build()
    with _lock:
        if _lib is not None:
            return _lib
        try:
            lib = C.CDLL(LIB_PATH)
        except OSError as e:  # fail loudly: there is no other implementation to fall back to
            raise CarcaHipError(f"cannot load {LIB_PATH}: {e}") from e
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.carca_abi_version() != 3:
            raise CarcaHipError("libcarca_hip.so ABI version mismatch")
        _lib = lib
        return lib


def check(rc: int, what: str) -> None:
    if rc == 0:
        return
    msg = load().carca_last_error().decode(errors="replace")
    kind = {-1: "unsupported configuration", -2: "bad argument"}.get(rc, f"hipError {rc}")
    raise CarcaHipError(f"{what}: {kind}: {msg}")
