"""Fused AdamW over a flat fp32 owner space.

Replaces ``torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=0.01)``
(train_harness.py:328-329) and DeepSpeed's FusedAdam (``"optimizer": {"type": "AdamW"}`` in
configs/deepspeed/zero{2,3}.json).  The rank's optimizer state — fp32 master weights, exp_avg,
exp_avg_sq — lives in three flat tensors; one HIP launch (csrc/adamw.hip) reads master/m/v/grad
once and writes master/m/v plus the bf16 compute copy of every parameter straight into its
destination (the replicated flat parameter buffer, or this rank's parameter shard).

``state="fp8"`` keeps the two moments as block-scaled OCP E4M3 codes: one byte per element for ``exp_avg`` and
for ``sqrt(exp_avg_sq)`` plus one fp32 power-of-two scale per 256 consecutive elements of a block-table row
(``[rows, 16]``), stochastically rounded with the counter hash of (seed, step count, owner index, moment) --
6 bytes per parameter and two small scale tables instead of 12.  The update itself stays fp32
(``adamw_fp8_kernel``; the contract is ``ops/ref.py`` ``adamw_flat_fp8``, which is also the CPU path).
"""
import math
from typing import List, Sequence, Tuple

import torch

from ..ops import ref
from ..ops._ext import ext


class FlatAdamW:
    def __init__(self, master: torch.Tensor, segments: Sequence[Tuple[int, int, torch.Tensor]],
                 lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, sub_group: int = 0,
                 state: str = "fp32", seed: int = 0):
        """``segments``: (owner_start, length, dst) with ``dst`` a contiguous 1-D view of length
        ``length`` receiving the compute-dtype copy of ``master[owner_start:owner_start+length]``.
        ``sub_group`` (DeepSpeed ZeRO-3 ``sub_group_size``, elements): update the owner space in
        launches of at most this many elements (0: one launch).  ``state``: ``fp32`` moments, or ``fp8``
        (block-scaled E4M3 codes, rounded with the random bits of ``seed`` and the step count)."""
        assert master.dtype == torch.float32 and master.dim() == 1
        if state not in ("fp32", "fp8"):
            raise ValueError(f"optimizer state must be fp32 or fp8, not {state!r}")
        self.master = master
        self.state = state
        self.fp8 = state == "fp8"
        self.seed = int(seed) & 0x7FFFFFFFFFFFFFFF
        self.rounding = "stochastic"     # "nearest" (the CPU reference only) shows why it is not used: an EMA stalls
        if self.fp8:
            self.exp_avg = torch.zeros(master.numel(), dtype=torch.uint8, device=master.device)
            self.exp_avg_sq = torch.zeros(master.numel(), dtype=torch.uint8, device=master.device)
        else:
            self.exp_avg = torch.zeros_like(master)
            self.exp_avg_sq = torch.zeros_like(master)
        self.exp_avg_scale = self.exp_avg_sq_scale = None     # fp8: [rows, 16] fp32, one per 256 elements of a row
        self.segments = list(segments)
        self.lr, self.betas, self.eps, self.weight_decay = lr, tuple(betas), eps, weight_decay
        self.step_count = 0
        self._lr_now = float(lr)
        self._tables = None
        self._seg_blocks = []    # segment -> (first, end) rows of the block tables (contiguous)
        self.sub_group = int(sub_group or 0)
        self._sub_ranges = None  # sub-group -> (first, end) rows of the block tables
        self.hp = None
        # compute-dtype copies written by the kernel: bf16 or fp16 (all segments share one)
        dts = {dst.dtype for _, _, dst in self.segments}
        assert len(dts) <= 1, "AdamW segments must share one compute dtype"
        self.dst_f16 = dts == {torch.float16}
        if master.is_cuda:
            self._build_tables()
            # fp8: hp[4] carries the launch counter (the step count) as integer bits
            self.hp = torch.zeros(5 if self.fp8 else 4, dtype=torch.float32, device=master.device)
        elif self.fp8:
            self._build_rows(ref.ADAM_CHUNK)
        if self.fp8:
            rows = self._seg_blocks[-1][1] if self._seg_blocks else 0
            self.exp_avg_scale = torch.ones(rows, ref.FP8_ROW_BLOCKS, dtype=torch.float32, device=master.device)
            self.exp_avg_sq_scale = torch.ones_like(self.exp_avg_scale)

    def _build_rows(self, chunk):
        """segment -> (first, end) rows of the block table (rows of ``chunk`` elements that never straddle a
        segment): all the CPU path of the fp8 state needs of the tables."""
        end = 0
        for ostart, length, dst in self.segments:
            first, end = end, end + (length + chunk - 1) // chunk
            self._seg_blocks.append((first, end))

    def _build_tables(self):
        chunk = ext().adamw_chunk()
        assert not self.fp8 or chunk == ref.ADAM_CHUNK, "the fp8 state's blocks are laid along 4096-element rows"
        blk_seg: List[int] = []
        blk_start: List[int] = []
        so, sl, sd = [], [], []
        for i, (ostart, length, dst) in enumerate(self.segments):
            assert dst.is_contiguous() and dst.numel() == length
            assert length % 4 == 0 and ostart % 4 == 0 and dst.data_ptr() % 8 == 0, "AdamW segments must be 4-aligned"
            so.append(ostart)
            sl.append(length)
            sd.append(dst.data_ptr())
            first = len(blk_seg)
            for s in range(ostart, ostart + length, chunk):
                blk_seg.append(i)
                blk_start.append(s)
            self._seg_blocks.append((first, len(blk_seg)))
        if self.sub_group > 0:
            per = max(1, self.sub_group // chunk)        # block-table rows per launch
            self._sub_ranges = [(lo, min(lo + per, len(blk_seg))) for lo in range(0, len(blk_seg), per)]
        dev = self.master.device
        self._tables = (torch.tensor(blk_seg, dtype=torch.int32, device=dev),
                        torch.tensor(blk_start, dtype=torch.int64, device=dev),
                        torch.tensor(so, dtype=torch.int64, device=dev),
                        torch.tensor(sl, dtype=torch.int64, device=dev),
                        torch.tensor(sd, dtype=torch.int64, device=dev))

    # ---- step-dependent hyper-parameters live on the device ([lr, lr/bc1, 1/sqrt(bc2)]) so a
    # captured HIP graph of the optimizer step stays valid across replays: ``prepare`` advances
    # the host step counter and uploads the values (skipped while a graph is being captured;
    # the graph runner calls ``upload`` before every replay).
    def prepare(self, lr: float):
        self.step_count += 1
        self._lr_now = float(lr)
        if self.master.is_cuda and not torch.cuda.is_current_stream_capturing():
            self.upload()

    def upload(self):
        b1, b2 = self.betas
        bc1 = 1.0 - b1 ** self.step_count
        bc2 = 1.0 - b2 ** self.step_count
        vals = (self._lr_now, self._lr_now / bc1, 1.0 / math.sqrt(bc2), 0.0)
        if self.hp.is_cuda:
            # one fill per value: the scalars travel as kernel arguments.  A copy_ from a (pageable)
            # host tensor would synchronize the stream -- a full pipeline drain at every window
            # boundary of an eager (multi-rank) run
            for i, v in enumerate(vals):
                self.hp[i:i + 1].fill_(v)
            if self.fp8:
                self.hp.view(torch.int32)[4:5].fill_(self._counter)
        else:
            self.hp.copy_(torch.tensor(vals))

    @property
    def _counter(self) -> int:
        """The launch counter of the fp8 state's random bits: the step count (31 bits, so it fits hp's int32 view)."""
        return self.step_count & 0x7FFFFFFF

    def _launch_fp8(self, lo, hi, grad, gscale, grid_cap=0):
        """Rows [lo, hi) of the block tables through ``adamw_fp8``; the scales are addressed by the global row."""
        b1, b2 = self.betas
        t = self._tables
        rows = (t[0], t[1]) if (lo == 0 and hi == t[0].numel()) else (t[0][lo:hi], t[1][lo:hi])
        ext().adamw_fp8(self.master, self.exp_avg, self.exp_avg_sq, self.exp_avg_scale, self.exp_avg_sq_scale, grad,
                        *rows, *t[2:], gscale, self._lr_now, b1, b2, self.eps, self.weight_decay, self.step_count,
                        self.hp, self.dst_f16, grid_cap, lo, self.seed, self._counter)

    def launch(self, grad: torch.Tensor, gscale: torch.Tensor = None):
        b1, b2 = self.betas
        if self._sub_ranges is not None and len(self._sub_ranges) > 1:
            for lo, hi in self._sub_ranges:
                self._launch_rows(lo, hi, grad, gscale)
            return
        if self.fp8:
            self._launch_fp8(0, self._tables[0].numel(), grad, gscale)
            return
        ext().adamw(self.master, self.exp_avg, self.exp_avg_sq, grad, *self._tables, gscale,
                    self._lr_now, b1, b2, self.eps, self.weight_decay, self.step_count, self.hp, self.dst_f16)

    @property
    def launches_per_step(self) -> int:
        return len(self._sub_ranges) if self._sub_ranges else 1

    def _launch_rows(self, lo, hi, grad, gscale, grid_cap=0):
        b1, b2 = self.betas
        if self.fp8:
            self._launch_fp8(lo, hi, grad, gscale, grid_cap)
            return
        ext().adamw(self.master, self.exp_avg, self.exp_avg_sq, grad, self._tables[0][lo:hi],
                    self._tables[1][lo:hi], *self._tables[2:], gscale,
                    self._lr_now, b1, b2, self.eps, self.weight_decay, self.step_count, self.hp, self.dst_f16,
                    grid_cap)

    def launch_segment(self, i: int, grad: torch.Tensor, gscale: torch.Tensor = None, grid_cap: int = 0):
        """The update of segment ``i`` alone (one launch over a slice of the block tables; the
        blocks of a segment are contiguous rows).  With ``prepare`` called once per step, the
        per-segment launches together are exactly ``launch`` -- the engine uses them to let each
        bucket's forward wait for its own parameters only.  ``grid_cap`` > 0 runs the rows on at most
        that many workgroups (a side-stream update that should leave the CUs to concurrent kernels)."""
        if not self.master.is_cuda:              # CPU reference: the same update on the segment's rows
            b1, b2 = self.betas
            ostart, length, dst = self.segments[i]
            sl = slice(ostart, ostart + length)
            if self.fp8:
                self._cpu_fp8_segment(i, grad, self._lr_now, gscale)
                dst.copy_(self.master[sl])
                return
            ref.adamw_flat(self.master[sl], self.exp_avg[sl], self.exp_avg_sq[sl], grad[sl], self._lr_now, b1, b2,
                           self.eps, self.weight_decay, self.step_count, gscale)
            dst.copy_(self.master[sl])
            return
        lo, hi = self._seg_blocks[i]
        self._launch_rows(lo, hi, grad, gscale, grid_cap)

    def _seg_scales(self, i):
        """Views of segment ``i``'s scales (its rows are contiguous and all but the last one full)."""
        nb = (self.segments[i][1] + ref.FP8_BLOCK - 1) // ref.FP8_BLOCK
        lo = self._seg_blocks[i][0] * ref.FP8_ROW_BLOCKS
        return self.exp_avg_scale.view(-1)[lo:lo + nb], self.exp_avg_sq_scale.view(-1)[lo:lo + nb]

    def _cpu_fp8_segment(self, i, grad, lr, gscale):
        b1, b2 = self.betas
        ostart, length, dst = self.segments[i]
        sl = slice(ostart, ostart + length)
        ms, ss = self._seg_scales(i)
        ref.adamw_flat_fp8(self.master[sl], self.exp_avg[sl], self.exp_avg_sq[sl], ms, ss, grad[sl], lr, b1, b2,
                           self.eps, self.weight_decay, self.step_count, gscale, seed=self.seed,
                           counter=self._counter, owner_off=ostart, rounding=self.rounding)

    @torch.no_grad()
    def step(self, grad: torch.Tensor, lr: float, gscale: torch.Tensor = None):
        assert grad.numel() == self.master.numel()
        b1, b2 = self.betas
        if self.master.is_cuda:
            self.prepare(lr)
            self.launch(grad, gscale)
            return
        self.step_count += 1
        if self.fp8:                            # segment by segment: the blocks lie along each segment's rows
            for i, (ostart, length, dst) in enumerate(self.segments):
                self._cpu_fp8_segment(i, grad, lr, gscale)
                dst.copy_(self.master[ostart:ostart + length])
            return
        n = self.master.numel()
        sg = self.sub_group if self.sub_group > 0 else n
        for lo in range(0, n, sg):              # sub-groups: same update, launch by launch
            hi = min(n, lo + sg)
            ref.adamw_flat(self.master[lo:hi], self.exp_avg[lo:hi], self.exp_avg_sq[lo:hi], grad[lo:hi], lr, b1,
                           b2, self.eps, self.weight_decay, self.step_count, gscale)
        for ostart, length, dst in self.segments:
            dst.copy_(self.master[ostart:ostart + length])

    def _dequantized(self):
        """fp8 state -> fp32 (exp_avg, exp_avg_sq) over the owner space (zeros outside the segments)."""
        m = torch.zeros_like(self.master)
        v = torch.zeros_like(self.master)
        for i, (ostart, length, dst) in enumerate(self.segments):
            sl = slice(ostart, ostart + length)
            ms, ss = self._seg_scales(i)
            if self.master.is_cuda:
                m[sl] = ext().fp8_dequantize(self.exp_avg[sl], ms)
                d = ext().fp8_dequantize(self.exp_avg_sq[sl], ss)
            else:
                m[sl] = ref.fp8_dequantize(self.exp_avg[sl], ms)
                d = ref.fp8_dequantize(self.exp_avg_sq[sl], ss)
            v[sl] = d * d
        return m, v

    def _quantize_from(self, exp_avg, exp_avg_sq):
        """fp32 moments -> the fp8 state, rounded to nearest.  Moments that came out of an fp8 state are exactly
        representable (a block whose scale halves doubles its codes), so they load value for value."""
        for i, (ostart, length, dst) in enumerate(self.segments):
            sl = slice(ostart, ostart + length)
            ms, ss = self._seg_scales(i)
            m = exp_avg[sl].to(self.master.device, torch.float32).contiguous()
            s = exp_avg_sq[sl].to(self.master.device, torch.float32).sqrt()
            for kind, val, codes, scales in ((ref.FP8_KIND_M, m, self.exp_avg[sl], ms),
                                             (ref.FP8_KIND_S, s, self.exp_avg_sq[sl], ss)):
                if self.master.is_cuda:
                    ext().fp8_quantize(val, kind, self.seed, 0, ostart, True, codes, scales)
                else:
                    c, sc = ref.fp8_quantize(val, kind, self.seed, 0, ostart, "nearest")
                    codes.copy_(c)
                    scales.copy_(sc)

    def state_dict(self):
        """The moments are fp32 under either state (``"state"`` names the one they came from), so a checkpoint
        loads into an optimizer of the other kind too."""
        m, v = self._dequantized() if self.fp8 else (self.exp_avg, self.exp_avg_sq)
        return {"step": self.step_count, "master": self.master, "exp_avg": m,
                "exp_avg_sq": v, "lr": self.lr, "betas": self.betas, "eps": self.eps,
                "weight_decay": self.weight_decay, "state": self.state}

    def load_state_dict(self, sd):
        self.step_count = int(sd["step"])
        self.master.copy_(sd["master"])
        if self.fp8:
            self._quantize_from(sd["exp_avg"], sd["exp_avg_sq"])
        else:
            self.exp_avg.copy_(sd["exp_avg"])
            self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        for ostart, length, dst in self.segments:
            dst.copy_(self.master[ostart:ostart + length])

    @property
    def state_bytes(self) -> int:
        n = self.master.numel()
        if self.fp8:                            # fp32 master, two code bytes, two [rows, 16] fp32 scale tables
            return n * 4 + 2 * n + 2 * self.exp_avg_scale.numel() * 4
        return 3 * n * 4
