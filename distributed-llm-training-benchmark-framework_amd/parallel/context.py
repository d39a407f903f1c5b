"""Context parallelism: one causal sequence split over the ``cp`` consecutive ranks of a group.

The scheme is the all-gather-KV one.  Every rank of a group draws the same rows and keeps the queries of its
*ranges* of each row; everything outside attention (norms, projections, MLP, head, loss) sees only those
``B * T / cp`` tokens, so to the strategy engines a context-parallel rank is one more data-parallel rank (equal
slices: the mean of the local mean losses is the global mean, and the engines average gradients as always).
Inside attention K | V of the local rows (after RoPE) are all-gathered over the group into a full-length buffer in
position order, the query-range kernels (``F_.attn_fwd(..., q_range=...)``, csrc/attention.hip) run the local
queries of each range against all ``T`` keys, and the backward reduce-scatters dK | dV back to the rows' owners.
No LSE merging, no ring.

Layouts (``ranges(layout, T, cp, r)``):

* ``contiguous``: rank r owns ``[r T/cp, (r+1) T/cp)``.  Even work under a sliding window, where every query
  block sees about the same number of keys.  ``T % (128 cp) == 0``.
* ``zigzag``: T is cut into ``2 cp`` chunks and rank r owns chunks r and ``2 cp - 1 - r``, which evens out the
  causal triangle (contiguous gives the last of 8 ranks 15/8 of the mean).  ``T % (256 cp) == 0``.  The kernels run
  once per chunk; the two dK | dV results (bf16, each zero outside the keys its chunk sees) are summed by one add
  before the reduce-scatter.

``auto`` is zigzag without a window and contiguous with one.

Local token order: a rank's tokens are laid out range-major, ``[range][batch row][position]`` -- to the model a
batch of ``n_ranges * B`` rows of ``T / (cp n_ranges)`` tokens -- so each range's Q / O / dO / dQ rows are one
contiguous block, which is what the range kernels take.  The gathered K | V rows are put into position order (and
dK | dV back into owner order) by one row gather each, with index tables built once per shape.

The group has a ``Comm`` of its own on its own process group, so K | V traffic does not queue behind the gradient
collectives of the engine's communicator.
"""
import torch
import torch.distributed as dist

from ..comm.collectives import Comm, emulated_world

LAYOUTS = ("contiguous", "zigzag")
BLOCK = 128          # the attention kernels' query block: every range bound is a multiple of it


def resolve_layout(layout, window=None):
    """``auto`` -> zigzag without a sliding window, contiguous with one."""
    if layout in (None, "auto"):
        return "contiguous" if window else "zigzag"
    if layout not in LAYOUTS:
        raise ValueError(f"context parallel: unknown layout {layout!r} (one of auto, {', '.join(LAYOUTS)})")
    return layout


def check_divisible(layout, T, cp):
    unit = BLOCK * cp * (2 if layout == "zigzag" else 1)
    if cp < 1:
        raise ValueError(f"context parallel: N must be >= 1, got {cp}")
    if cp > 1 and T % unit:
        raise ValueError(f"context parallel: the {layout} layout over {cp} ranks needs a sequence length that is a "
                         f"multiple of {unit} ({BLOCK * (2 if layout == 'zigzag' else 1)} x {cp}), got {T}")


def ranges(layout, T, cp, r):
    """The query ranges ``[(begin, end), ...]`` of group rank ``r``, in position order."""
    check_divisible(layout, T, cp)
    if not 0 <= r < cp:
        raise ValueError(f"context parallel: rank {r} outside the group of {cp}")
    if cp == 1:
        return [(0, T)]
    if layout == "contiguous":
        n = T // cp
        return [(r * n, (r + 1) * n)]
    n = T // (2 * cp)
    return [(r * n, (r + 1) * n), ((2 * cp - 1 - r) * n, (2 * cp - r) * n)]


def visible_pairs(rngs, T, window=None):
    """(query, key) pairs the queries of ``rngs`` see under the causal mask (and a window W: i - W < j <= i)."""
    total = 0
    for b, e in rngs:
        for i in (b, e - 1):
            assert 0 <= i < T
        if window and 0 < window < T:
            # sum over i in [b, e) of min(i + 1, W)
            k = min(max(window - 1, b), e)          # queries below k see i + 1 keys, the rest W
            total += (b + 1 + k) * (k - b) // 2 + (e - k) * window
        else:
            total += (b + 1 + e) * (e - b) // 2
    return total


def check_world(cp, world):
    if cp < 1 or world % cp:
        raise ValueError(f"--context-parallel {cp} must divide the world size {world}")


class ContextParallel:
    """The context-parallel group of this rank: its layout, ranges and communicator.  ``attach(model)`` makes a
    Mistral-shape model slice its rows and run attention through the group."""

    def __init__(self, cp, layout="auto", window=None, world=None, rank=None):
        ready = dist.is_available() and dist.is_initialized()
        self.world = (dist.get_world_size() if ready else 1) if world is None else world
        self.global_rank = (dist.get_rank() if ready else 0) if rank is None else rank
        check_world(cp, self.world)
        if cp > 1 and emulated_world():
            raise ValueError("context parallelism cannot run on the emulated fabric (DLTB_COMM=emulate:N models one "
                             "group only)")
        self.cp = cp
        self.layout = resolve_layout(layout, window)
        self.group_index, self.rank = divmod(self.global_rank, cp)
        self.dp_world = self.world // cp          # groups: the data-parallel width the batcher sees
        group = None
        if cp > 1:
            if not ready:
                raise ValueError("context parallelism needs an initialised process group")
            for g in range(self.world // cp):      # every rank creates every group, in the same order
                pg = dist.new_group(list(range(g * cp, (g + 1) * cp)))
                if g == self.group_index:
                    group = pg
        self.comm = Comm(group) if cp > 1 else None
        self._index = {}

    def ranges(self, T):
        return ranges(self.layout, T, self.cp, self.rank)

    def local_len(self, T):
        return T // self.cp

    def attach(self, model):
        cfg = getattr(model, "cfg", None)
        if cfg is None or not getattr(cfg, "causal", False) or not hasattr(model, "rope"):
            raise ValueError("context parallelism needs a causal Mistral-shape tier (M7B, M7B_narrow, mtiny); the "
                             "TinyGPT tiers attend non-causally, with dropout and learned positions")
        model.cp = self if self.cp > 1 else None
        return model

    def describe(self, T):
        return {"context_parallel": self.cp, "cp_layout": self.layout,
                "cp_ranges": [[list(x) for x in ranges(self.layout, T, self.cp, r)] for r in range(self.cp)]}

    # ---------------------------------------------------------------------------------------- token layout
    def slice_rows(self, x, T):
        """``x`` [B, T, ...] -> this rank's tokens, range-major: [n_ranges * B, T / (cp n_ranges), ...]."""
        assert x.shape[1] == T
        return torch.cat([x[:, b:e] for b, e in self.ranges(T)], 0).contiguous()

    def rope_rows(self, cos, sin, T):
        """The cos / sin rows of each range's positions (views of the position-indexed tables)."""
        return [(cos[b:e], sin[b:e]) for b, e in self.ranges(T)]

    def _tables(self, B, T, device):
        """(to_pos, to_owner): row gathers between owner order -- [group rank][range][b][t], what all_gather
        produces and reduce_scatter consumes -- and position order [b][position]."""
        key = (B, T, str(device))
        if key not in self._index:
            src = torch.empty(B, T, dtype=torch.int64)
            per = B * (T // self.cp)
            for r in range(self.cp):
                row = r * per
                for b, e in ranges(self.layout, T, self.cp, r):
                    n = e - b
                    src[:, b:e] = row + torch.arange(B)[:, None] * n + torch.arange(n)[None, :]
                    row += B * n
            to_pos = src.reshape(-1)
            to_owner = torch.empty_like(to_pos)
            to_owner[to_pos] = torch.arange(B * T)
            self._index[key] = (to_pos.to(device), to_owner.to(device))
        return self._index[key]

    # ---------------------------------------------------------------------------------------- K | V traffic
    def gather_kv(self, kv_local, B, T):
        """K | V of the local rows ([n_local, C], any row stride) -> [B * T, C] in position order.  The gather is
        issued asynchronously on the group's communicator and waited for here, before any kernel reads it."""
        local = kv_local.contiguous()
        owner = torch.empty(self.cp * local.shape[0], local.shape[1], dtype=local.dtype, device=local.device)
        self.comm.all_gather(owner, local, async_op=True, track=False).wait()
        return owner.index_select(0, self._tables(B, T, local.device)[0])

    def scatter_dkv(self, dkv_full, out_local, B, T):
        """dK | dV of all T rows (this rank's queries' contribution, [B * T, C]) -> summed over the group, this
        rank's rows into ``out_local`` ([n_local, C], any row stride).  Waited for before it is consumed."""
        owner = dkv_full.index_select(0, self._tables(B, T, dkv_full.device)[1])
        mine = torch.empty(owner.shape[0] // self.cp, owner.shape[1], dtype=owner.dtype, device=owner.device)
        self.comm.reduce_scatter(mine, owner, async_op=True, track=False).wait()
        out_local.copy_(mine)
