"""Plain-torch reference of the binning csmoe_decode_route leaves behind: the stable counting sort of csmoe_bin_tokens, by
torch.sort(stable=True).  Ids outside [0, E) are skipped (their perm / slot_of entries are unspecified: -1 here)."""
import torch


def ref_bins(idx: torch.Tensor, E: int):
    """idx [T, K] (any int dtype, any device) -> (counts [E], offsets [E+1], perm [n], slot_of [n]) int32 on the CPU.  `perm` is
    filled for the offsets[E] valid ids only; the rest of it, and slot_of of a skipped id, is -1."""
    flat = idx.reshape(-1).cpu().long()
    n = flat.numel()
    valid = (flat >= 0) & (flat < E)
    key = torch.where(valid, flat, torch.full_like(flat, E))           # skipped ids sort behind every expert
    order = torch.sort(key, stable=True).indices
    nv = int(valid.sum())
    counts = torch.bincount(flat[valid], minlength=E)[:E]
    offsets = torch.zeros(E + 1, dtype=torch.long)
    offsets[1:] = torch.cumsum(counts, 0)
    perm = torch.full((n,), -1, dtype=torch.long)
    perm[:nv] = order[:nv]
    slot_of = torch.full((n,), -1, dtype=torch.long)
    slot_of[order[:nv]] = torch.arange(nv)
    return counts.int(), offsets.int(), perm.int(), slot_of.int()
