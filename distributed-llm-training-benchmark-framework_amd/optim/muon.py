"""Muon over the hidden matrices of a flat fp32 owner space, AdamW over everything else.

Muon (``--optimizer muon``): Nesterov momentum, the result orthogonalised by five quintic Newton-Schulz
iterations, scaled by ``0.2 sqrt(max(rows, cols))`` so its RMS matches an AdamW update and ``lr`` /
``weight_decay`` keep their meaning.  The contract -- constants and rounding points -- is
``ops/ref.py`` ``muon_momentum`` / ``muon_newton_schulz`` / ``muon_update``, which is also the CPU path.

On the GPU (csrc/muon.hip) one optimizer step is

    muon_momentum                  every matrix: momentum, the bf16 operand U (transposed to m <= n), 1 / ||U||
    per shape (m, n), ns_steps x   muon_syrk  A = s^2 X X^T      (lower-triangle tiles: half the MFMA work)
                                   muon_syrk  B = b A + c A A
                                   muon_apply X' = s (a X + B X)
    muon_update                    every matrix: master weights and their compute-dtype copy
    adamw                          the complement of the matrices in the owner space (the inner ``FlatAdamW``)

with the matrices of one (m, n) -- all layers, and both orientations -- stacked in one work buffer so that each
product is ONE batched launch.
"""
from typing import List, Sequence, Tuple

import torch

from ..ops import ref
from ..ops._ext import ext
from .adamw import FlatAdamW

TILE = 64


def muon_matrices(model) -> List[tuple]:
    """(unit, index, name, shape) of the parameters Muon updates: every 2-D parameter of a transformer block whose
    two dimensions are multiples of 64, as the model stores it (fused QKV and gate/up are one matrix each), except
    the MoE router, linear attention's decay gate and the expert weights.  Embeddings, the LM head, norms, biases,
    sinks stay on AdamW."""
    out = []
    for u in model.unit_blocks:
        for i, (name, p) in enumerate(zip(u.names, u.params)):
            if p.dim() == 2 and p.shape[0] % TILE == 0 and p.shape[1] % TILE == 0 \
                    and ".router." not in name and ".decay_gate." not in name and ".experts." not in name:
                out.append((u, i, name, tuple(p.shape)))
    return out


def complement_segments(segments, ranges):
    """``segments`` (owner_start, length, dst) minus the owner ranges ``ranges`` [(start, end)], each of which must lie
    inside one segment."""
    ranges = sorted(ranges)
    out, k = [], 0
    for ostart, length, dst in sorted(segments, key=lambda s: s[0]):
        pos, end = ostart, ostart + length
        while k < len(ranges) and ranges[k][0] < end:
            lo, hi = ranges[k]
            if lo < pos or hi > end:
                raise ValueError("--optimizer muon needs every Muon matrix whole inside the rank's owner space")
            if lo > pos:
                out.append((pos, lo - pos, dst[pos - ostart:lo - ostart]))
            pos = hi
            k += 1
        if end > pos:
            out.append((pos, end - pos, dst[pos - ostart:end - ostart]))
    if k != len(ranges):
        raise ValueError("--optimizer muon needs every Muon matrix whole inside the rank's owner space")
    return out


class FlatMuon:
    def __init__(self, master: torch.Tensor, segments: Sequence[Tuple[int, int, torch.Tensor]],
                 matrices: Sequence[Tuple[str, tuple, int, torch.Tensor]], lr=1e-4, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=0.01, momentum=ref.MUON_MOMENTUM, ns_steps=ref.MUON_NS_STEPS, state: str = "fp32",
                 seed: int = 0):
        """``segments`` as for :class:`FlatAdamW` (the whole owner space); ``matrices``: (name, (rows, cols),
        owner_start, dst) with ``dst`` the contiguous compute-dtype copy of that matrix.  ``state`` (fp32 | fp8
        moments) applies to the inner AdamW only; the Muon momentum is fp32."""
        if int(ns_steps) < 1:
            raise ValueError("muon_ns_steps must be >= 1")
        for name, (rows, cols), ostart, dst in matrices:
            if rows % TILE or cols % TILE or dst.numel() != rows * cols or not dst.is_contiguous():
                raise ValueError(f"Muon matrix {name}: dimensions must be multiples of {TILE}")
        # stacked by work shape (m <= n): every product of a shape is one batched launch
        kinds = {}
        for mt in matrices:
            kinds.setdefault((min(mt[1]), max(mt[1])), []).append(mt)
        self._kinds = [(k, len(v)) for k, v in kinds.items()]
        self._mats = [mt for v in kinds.values() for mt in v]
        self.master = master
        self.momentum, self.ns_steps = float(momentum), int(ns_steps)
        self.lr, self.weight_decay = lr, weight_decay
        self.inner = FlatAdamW(master, complement_segments(segments, [(o, o + r * c) for _, (r, c), o, _ in self._mats]),
                               lr, betas, eps, weight_decay, state=state, seed=seed)
        n = sum(r * c for _, (r, c), _, _ in self._mats)
        self.mom = torch.zeros(n, dtype=torch.float32, device=master.device)
        self._offs = []                  # per matrix: offset in ``mom`` and in the stacked work buffers
        off = 0
        for _, (r, c), _, _ in self._mats:
            self._offs.append(off)
            off += r * c
        if master.is_cuda:
            self._build_tables()

    matrices = property(lambda self: [(name, shape) for name, shape, _, _ in self._mats])
    # what the engines read of an optimizer
    hp = property(lambda self: self.inner.hp)
    betas = property(lambda self: self.inner.betas)
    state = property(lambda self: self.inner.state)
    fp8 = property(lambda self: self.inner.fp8)
    sub_group = 0

    # the step count and the current lr are the inner optimizer's (the graph runner saves and restores both)
    @property
    def step_count(self):
        return self.inner.step_count

    @step_count.setter
    def step_count(self, v):
        self.inner.step_count = v

    @property
    def _lr_now(self):
        return self.inner._lr_now

    @_lr_now.setter
    def _lr_now(self, v):
        self.inner._lr_now = v

    def _build_tables(self):
        dev = self.master.device
        for _, _, _, dst in self._mats:
            if dst.dtype != torch.bfloat16:
                raise ValueError("--optimizer muon: the GPU kernels are bf16 (no fp16 operands)")
        tab, blk_mat, blk_tile = [], [], []
        for i, (name, (r, c), ostart, dst) in enumerate(self._mats):
            nb = (r // TILE) * (c // TILE)
            tab.append([r, c, ostart, self._offs[i], self._offs[i], dst.data_ptr(), len(blk_mat), nb])
            blk_mat += [i] * nb
            blk_tile += range(nb)
        self._tab_host = torch.tensor(tab, dtype=torch.int64).reshape(-1, 8)
        self._tab = self._tab_host.to(dev)
        self._blk = (torch.tensor(blk_mat, dtype=torch.int32, device=dev),
                     torch.tensor(blk_tile, dtype=torch.int32, device=dev))
        n = self.mom.numel()
        self._x = [torch.zeros(n, dtype=torch.bfloat16, device=dev) for _ in range(2)]     # X ping-pong (U first)
        sq = max((cnt * m * m for (m, _), cnt in self._kinds), default=0)
        self._ab = [torch.zeros(sq, dtype=torch.bfloat16, device=dev) for _ in range(2)]   # A and B of one shape
        self._partial = torch.zeros(max(1, len(blk_mat)), dtype=torch.float32, device=dev)
        self.norms = torch.zeros(max(1, len(self._mats)), 2, dtype=torch.float32, device=dev)   # (s, s^2) per matrix

    # ---- the FlatAdamW interface of the engines
    def prepare(self, lr: float):
        self.inner.prepare(lr)

    def upload(self):
        self.inner.upload()

    @property
    def launches_per_step(self) -> int:
        return 3 + 3 * self.ns_steps * len(self._kinds) + self.inner.launches_per_step

    def launch(self, grad: torch.Tensor, gscale: torch.Tensor = None):
        C = ext()
        a, b, c = ref.MUON_ABC
        tabs = (self._tab, self._tab_host, *self._blk)
        if self._mats:
            C.muon_momentum(grad, self.mom, self._x[0], self._partial, self.norms, *tabs, gscale, self.hp,
                            self.momentum, ref.MUON_EPS)
            off = first = 0
            for (m, n), cnt in self._kinds:
                X, Y = (t[off:off + cnt * m * n].view(cnt, m, n) for t in self._x)
                A, B = (t[:cnt * m * m].view(cnt, m, m) for t in self._ab)
                s = self.norms[first:first + cnt]
                for i in range(self.ns_steps):
                    C.muon_syrk(X, A, None, 1.0, 0.0, s[:, 1] if i == 0 else None)
                    C.muon_syrk(A, B, A, c, b)
                    C.muon_apply(B, X, Y, 1.0, a, s[:, 0] if i == 0 else None)
                    X, Y = Y, X
                off += cnt * m * n
                first += cnt
            C.muon_update(self.master, self._x[self.ns_steps % 2], *tabs, self.hp, self._lr_now,
                          self.weight_decay)
        self.inner.launch(grad, gscale)

    def launch_segment(self, *a, **k):
        raise RuntimeError("FlatMuon updates whole matrices after the last reduction: no per-segment launches")

    @torch.no_grad()
    def step(self, grad: torch.Tensor, lr: float, gscale: torch.Tensor = None):
        assert grad.numel() == self.master.numel()
        if self.master.is_cuda:
            self.prepare(lr)
            self.launch(grad, gscale)
            return
        for (name, (r, c), ostart, dst), moff in zip(self._mats, self._offs):
            sl = slice(ostart, ostart + r * c)
            U, s = ref.muon_momentum(self.mom[moff:moff + r * c].view(r, c), grad[sl].view(r, c), self.momentum, gscale)
            w = self.master[sl].view(r, c)
            ref.muon_update(w, ref.muon_newton_schulz(U, s, self.ns_steps), lr, self.weight_decay)
            dst.view(r, c).copy_(w)
        self.inner.step_count += 1       # the inner update segment by segment: its CPU ``step`` walks the whole master
        self.inner._lr_now = float(lr)
        for i in range(len(self.inner.segments)):
            self.inner.launch_segment(i, grad, gscale)

    def state_dict(self):
        sd = self.inner.state_dict()
        sd.update(optimizer="muon", muon_momentum=self.mom, muon_matrices=self.matrices)
        return sd

    def load_state_dict(self, sd):
        if "muon_momentum" not in sd or sd["muon_momentum"].numel() != self.mom.numel():
            raise ValueError("checkpoint holds no matching Muon momentum (written with another --optimizer?)")
        self.inner.load_state_dict(sd)
        self.mom.copy_(sd["muon_momentum"])
        for name, (r, c), ostart, dst in self._mats:
            dst.view(-1).copy_(self.master[ostart:ostart + r * c])

    @property
    def state_bytes(self) -> int:
        return self.inner.state_bytes + self.mom.numel() * 4

    @property
    def work_bytes(self) -> int:
        """bf16 Newton-Schulz scratch (two X buffers, A and B), not optimizer state."""
        if not self.master.is_cuda:
            return 0
        return 2 * sum(t.numel() for t in self._x + self._ab)
