"""The row product of csrc/gemm*.hip stated once in plain torch (no kernel of this package), for tests/test_hip_gemm_matrix.py.

For one segment, in the order of csrc/gemm_epilogue.h:

    v = alpha (A0 B0^T + A1 B1^T) + bias + pos[row % T] + add + add_table[id] + rowscale[row] colvec
    v *= gate > 0 ? gs : ((gate < 0 or not gate_zero_drops) ? slope gs : 0)            gs = gate_scale or 1
    v  = 0 where mask_rows and id == 0;   columns N .. ncols_out - 1 = 0

alpha = 0 means 1.  The arguments are those of ops.gemm_rows (ops._gemm_desc): the segment is the same dict, the keywords the
same keywords.  dtype and device follow bt0, so the same code gives the float64 reference and the float32 one (see cast())."""
import torch


K_CHAIN = 1024


def product(a, bt):
    """a bt^T [rows, N]; for K > K_CHAIN the sum over K is taken in chains of K_CHAIN terms whose partial products are then
    added.  In float64 the grouping changes nothing that matters.  In float32 it keeps the yardstick sane: the test file
    demands noise <= 16 eps32 max|ref64| of it, and ATen's GPU product, one chain over all of K, measured 16.3 .. 19 at
    K = 2054 on an MI355X (2.4 on a CPU).  1024 is the longest power of two that keeps the bound there (two chains at
    K = 2054: 9.6 .. 11.5; 512: 5.4; 256: 3.3) -- chosen from the yardstick's own error, and the closest to the plain
    product, which it is for every K <= 1024."""
    K = a.shape[1]
    acc = None
    for k in range(0, K, K_CHAIN):
        p = a[:, k:k + K_CHAIN] @ bt[:, k:k + K_CHAIN].T
        acc = p if acc is None else acc + p
    return acc


def _f32(x):
    """A scalar as the kernels receive it (CarcaGemmDesc holds floats)."""
    return float(torch.tensor(float(x), dtype=torch.float32))


def operand_rows(t, K, ids=None, gather=False):
    """The [rows, K] matrix behind one of _gemm_desc's three operand forms: a 2-D view with lda >= K, a [B, T, K] view with
    strided users, or (gather) a table whose row ids[r] is row r."""
    if gather:
        return t[ids.reshape(-1).long()][:, :K]
    if t.dim() == 3:
        return t.reshape(-1, t.shape[2])[:, :K]
    return t[:, :K]


def gemm_rows_statement(seg, bt0, N, K0, *, bt1=None, K1=0, bias=None, pos=None, colvec=None, gate_slope=0.01,
                        mask_rows=False, ncols_out=None, gate_scale=1.0, gate_zero_drops=False, alpha=1.0, add_table=None):
    """-> [rows, ncols_out] (ncols_out defaults to N here; ops.gemm_rows defaults it to out_ld)."""
    dt = bt0.dtype
    ids = seg.get("ids")
    ids = ids.reshape(-1).long() if ids is not None else None
    a0 = operand_rows(seg["a0"], K0, ids, bool(seg.get("a0_gather")))
    v = product(a0, bt0[:, :K0])
    if K1:
        v = v + product(operand_rows(seg["a1"], K1), bt1[:, :K1])
    rows = v.shape[0]
    alpha = _f32(alpha)
    if alpha != 0.0:
        v = alpha * v
    if bias is not None:
        v = v + bias
    if seg.get("add_pos"):
        T = int(seg.get("T") or (seg["a0"].shape[1] if seg["a0"].dim() == 3 else 1))
        v = v + pos[torch.arange(rows, device=v.device) % T][:, :N]
    if seg.get("add") is not None:
        v = v + seg["add"][:, :N]
    if add_table is not None:
        v = v + add_table[ids][:, :N]
    if seg.get("rowscale") is not None:
        v = v + seg["rowscale"].reshape(-1, 1) * colvec.reshape(1, -1)
    if seg.get("gate") is not None:
        gate = seg["gate"][:, :N]
        gs = _f32(gate_scale) if _f32(gate_scale) != 0.0 else 1.0
        low = torch.tensor(_f32(gate_slope), dtype=dt, device=v.device) * torch.tensor(gs, dtype=dt, device=v.device)
        high = torch.tensor(gs, dtype=dt, device=v.device)
        zero = torch.zeros((), dtype=dt, device=v.device)
        m = torch.where(gate > 0, high, torch.where((gate < 0) | (not gate_zero_drops), low, zero))
        v = v * m
    if mask_rows:
        v = torch.where((ids != 0).unsqueeze(1), v, torch.zeros((), dtype=dt, device=v.device))
    ncols_out = N if ncols_out is None else ncols_out
    if ncols_out > N:
        v = torch.cat([v, torch.zeros(rows, ncols_out - N, dtype=dt, device=v.device)], dim=1)
    return v


def exact_zero(seg, N, *, mask_rows=False, ncols_out=None, gate_zero_drops=False, **_):
    """bool [rows, ncols_out]: where the statement gives an exact 0 whatever the operands hold -- masked rows, pad columns,
    dropped gates."""
    ids = seg.get("ids")
    rows = ids.numel() if ids is not None else (seg["a0"].shape[0] * seg["a0"].shape[1] if seg["a0"].dim() == 3 else seg["a0"].shape[0])
    ncols_out = N if ncols_out is None else ncols_out
    dev = seg["a0"].device
    z = torch.zeros(rows, ncols_out, dtype=torch.bool, device=dev)
    z[:, N:] = True
    if mask_rows:
        z |= (ids.reshape(-1) == 0).unsqueeze(1)
    if seg.get("gate") is not None and gate_zero_drops:
        z[:, :N] |= seg["gate"][:, :N] == 0
    return z


def cast(x, dtype):
    """The same arguments with every floating tensor in `dtype` (strides are not kept: the statement needs none)."""
    if isinstance(x, torch.Tensor):
        return x.to(dtype) if x.is_floating_point() else x
    if isinstance(x, dict):
        return {k: cast(v, dtype) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(cast(v, dtype) for v in x)
    return x
