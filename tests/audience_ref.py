"""A pure-torch reference of the running state behind CARCA.recommend_users (catalogue.AudienceTopK; DESIGN.md section
24): the 64-bit keys and their merge, on whatever device the tensors live.  A key sits in an int64 tensor as its raw bits:
the high word is the logit's order-preserving bits (csrc/recommend_common.h: rc::order_bits), the low word 0xFFFFFFFF minus
the user id, 0 is an empty entry; keys order as UNSIGNED integers, so every sort here goes through flip()."""
import torch

LOW = 0xFFFFFFFF
SIGN = -(1 << 63)            # the top bit of an int64: x ^ SIGN orders signed as x orders unsigned
SENTINEL_BITS = -1           # int32 view of 0xFFFFFFFF, the exclusion sentinel: order bits 0


def order_bits(logits: torch.Tensor) -> torch.Tensor:
    """float32 -> int64 in [0, 2^32): larger float, larger value; -0 orders just below +0; the sentinel gives 0."""
    b = logits.contiguous().view(torch.int32).to(torch.int64) & LOW
    return torch.where((b >> 31) != 0, ~b & LOW, b | 0x80000000)


def unorder_bits(o: torch.Tensor) -> torch.Tensor:
    b = torch.where((o >> 31) != 0, o & 0x7FFFFFFF, ~o & LOW)
    return torch.where(b >= 1 << 31, b - (1 << 32), b).to(torch.int32).view(torch.float32)


def pack(logits: torch.Tensor, users: torch.Tensor) -> torch.Tensor:
    """(float32 logits, int64 user ids in [0, 2^31)) -> keys, broadcast together."""
    return (order_bits(logits) << 32) | (LOW - users.to(torch.int64))  # (the shift wraps into the sign bit: raw bits)


def unpack(keys: torch.Tensor):
    """keys -> (float32 logits, int64 users, bool empty); an empty entry reads as logit 0 and user -1."""
    empty = keys == 0
    hi, lo = (keys >> 32) & LOW, keys & LOW
    logits = torch.where(empty, torch.zeros((), dtype=torch.float32), unorder_bits(hi))
    return logits, torch.where(empty, torch.full_like(lo, -1), LOW - lo), empty


def flip(keys: torch.Tensor) -> torch.Tensor:
    return keys ^ SIGN


def sort_desc(keys: torch.Tensor) -> torch.Tensor:
    """Every row of keys [Q, n] descending as unsigned integers (zeros last)."""
    return flip(torch.sort(flip(keys), dim=1, descending=True).values)


def new_keys(logits: torch.Tensor, users: torch.Tensor, eligible=None) -> torch.Tensor:
    """The keys a batch offers, item-major: logits [B, Q] raw float32, users [B] -> [Q, B]; 0 where the pair is not
    eligible: eligible [B, Q] is False, the user id is negative, or the logit holds the exclusion sentinel."""
    users = users.to(torch.int64)
    keys = pack(logits, users.clamp(min=0).unsqueeze(1))
    dead = (users < 0).unsqueeze(1) | (order_bits(logits) == 0)
    if eligible is not None:
        dead = dead | ~eligible
    return torch.where(dead, torch.zeros_like(keys), keys).t().contiguous()


def merge(old: torch.Tensor, logits: torch.Tensor, users: torch.Tensor, eligible=None) -> torch.Tensor:
    """One update: the k largest of a row's old keys and the batch's keys, as a sort of old U new.  old [Q, k]."""
    k = old.shape[1]
    return sort_desc(torch.cat([old, new_keys(logits, users, eligible)], dim=1))[:, :k].contiguous()


def link(logits: torch.Tensor, decoder: int) -> torch.Tensor:
    return (logits + 1) * 0.5 if decoder == 2 else torch.sigmoid(logits)
