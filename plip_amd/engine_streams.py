"""Which stream an engine's work runs on: the measured partner stream of ``encode_pair``, the lanes (an engine and a clone of it on two
streams) and the chunk loop of the encode entries.  Mixed into ``plip_amd.engine.Engine``; the per-engine state it reads and writes
(``_lanes``, ``_no_lanes``, ``_vis``, ``pair_stream_ratio``) is declared in ``Engine._init_own_state``."""
from __future__ import annotations

import contextlib
import ctypes as C
import itertools
from typing import Optional

import torch

from . import _lib

_SIDE_STREAMS = {}      # device -> the process's first ordinary stream, the first candidate below (created with the first engine)
_PAIR_STREAMS = {}      # (device, main stream) -> the text tower's stream of Engine.encode_pair, CHECKED to overlap with that main stream


class StreamsMixin:
    use_lanes = True        # a call of more than max_batch rows runs its chunks alternately on this engine and on a clone (``lanes``)

    def streams_overlap(self, a: "torch.cuda.Stream", b: "torch.cuda.Stream") -> float:
        """include/plipmi.h plipmi_streams_overlap: about 1 when kernels of ``a`` and ``b`` run side by side, about 2 when the two
        streams share a hardware queue (one waits for the other).  Synchronises both."""
        r = C.c_float(0.0)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.plipmi_streams_overlap(self._h, C.c_void_p(a.cuda_stream), C.c_void_p(b.cuda_stream), C.byref(r)),
                       "plipmi_streams_overlap")
        return float(r.value)

    def pair_stream(self, main: "torch.cuda.Stream") -> "torch.cuda.Stream":
        """The stream ``encode_pair`` runs the text tower on while the vision tower runs on ``main``: the process's first ordinary
        stream if it overlaps with ``main`` (it does in a process that created no streams before the engine -- the bench), otherwise
        the first of a few fresh ones that does; measured once per (device, main stream), about a millisecond each."""
        key = (self.device, main.cuda_stream)
        side = _PAIR_STREAMS.get(key)
        if side is None:
            tried = []
            for k in range(8):
                cand = _SIDE_STREAMS[self.device] if k == 0 and self.device in _SIDE_STREAMS else torch.cuda.Stream(device=self.device)
                ratio = 2.0 if cand.cuda_stream == main.cuda_stream else self.streams_overlap(main, cand)
                tried.append((ratio, k, cand))          # every candidate stays alive until the choice: fresh ones then differ
                if ratio < 1.5:
                    break
            self.pair_stream_ratio, _, side = min(tried, key=lambda t: t[:2])
            _PAIR_STREAMS[key] = side
        return side

    def lanes(self, n: int = 2):
        """``[(engine, stream), ...]`` for a loop over MANY batches of one tower: lane 0 is this engine on the caller's stream, lane 1
        a clone (made on first use, kept) on the stream ``pair_stream`` measured to run beside it.  Give batch k to lane k % n inside
        ``torch.cuda.stream(stream)`` and call ``join_lanes`` before the outputs are used on the caller's stream: the launch boundaries,
        epilogues and the pooled tail of one batch then run under the next batch's GEMMs (configs[3]'s shard: 99 -> 107 k img/s).  Every
        lane waits for the work the caller's stream holds at THIS call (inputs produced there are ready)."""
        main = torch.cuda.current_stream(self.device)
        if n <= 1:
            return [(self, main)]
        if self._lanes is None:
            self._lanes = [self.clone()]
        side = self.pair_stream(main)
        side.wait_stream(main)
        return [(self, main), (self._lanes[0], side)]

    @contextlib.contextmanager
    def lane_loop(self):
        """For host loops over many batches of one tower::

            with eng.lane_loop() as run:
                for batch in batches:
                    outs.append(run(lambda e: e.encode_image_u8(batch)))

        ``run`` gives consecutive calls to alternating lanes (``lanes``) and the block's exit joins them; with ``use_lanes`` off (or
        inside ``encode_pair`` / ``profile``) every call runs on this engine and the caller's stream, as a plain loop would."""
        lanes = self.lanes() if (self.use_lanes and not self._no_lanes) else [(self, None)]
        k = itertools.count()
        main = torch.cuda.current_stream(self.device)

        def run(fn):
            eng, st = lanes[next(k) % len(lanes)]
            if st is None:
                return fn(eng)
            with torch.cuda.stream(st):
                out = fn(eng)
            if torch.is_tensor(out):
                out.record_stream(main)
            return out

        self._no_lanes += 1         # the calls inside are single lanes: no fan-out of a lane's own chunks
        try:
            yield run
        finally:
            self._no_lanes -= 1
            if len(lanes) > 1:
                self.join_lanes(lanes)

    def join_lanes(self, lanes):
        """The caller's stream waits for every lane: outputs of all batches may be used on it afterwards."""
        main = torch.cuda.current_stream(self.device)
        for _, st in lanes[1:]:
            main.wait_stream(st)

    def _run_chunks(self, n: int, call, *args):
        """``call(engine, a, b, *args)`` for rows a..b of every chunk of at most ``max_batch`` rows.  A call of several chunks is a corpus
        walked through one tower: its chunks go alternately to the two ``lanes``, joined at the end (+8 % on configs[3]'s shard); a
        row's bits do not depend on the lane."""
        chunks = self._chunks(n)
        if len(chunks) < 2 or not self.use_lanes or self._no_lanes:
            for a, b in chunks:
                call(self, a, b, *args)
            return
        lanes = self.lanes()
        for k, (a, b) in enumerate(chunks):
            eng, st = lanes[k % len(lanes)]
            with torch.cuda.stream(st):
                call(eng, a, b, *args)
        self.join_lanes(lanes)

    def encode_pair(self, pixels: torch.Tensor, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                    normalize: bool = True, overlap: bool = True):
        """Both towers of one step.  With ``overlap`` the text tower is enqueued on a second HIP stream:
        the towers are independent (separate workspaces), so the tail of one tower's GEMM grid -- 150..600
        workgroups over 256 CUs -- is filled by the other tower's kernels instead of idling."""
        self._no_lanes += 1         # the second stream belongs to the other tower here (four towers at once measured +10 %)
        try:
            return self._encode_pair(pixels, input_ids, attention_mask, normalize, overlap)
        finally:
            self._no_lanes -= 1

    def _encode_pair(self, pixels, input_ids, attention_mask, normalize, overlap):
        ih, iw = self.image_hw  # the image side's shape error comes first, as in CLIPModel.forward, and before anything is enqueued
        ok = (tuple(pixels.shape[1:]) == (ih, iw, 3)) if pixels.dtype == torch.uint8 else \
            (pixels.dim() == 4 and tuple(pixels.shape[1:]) == (3, ih, iw))
        if not ok:
            self._encode_image_any(pixels, normalize)       # raises the tower's own ValueError
        n = pixels.shape[0]
        if overlap and self.pass_batch > 0 and n >= 2 * self.pass_batch and input_ids.shape[0] == n:
            # plipmi_config.pass_batch at the level that owns BOTH streams: equal passes, the two towers of a pass joined before the next
            # one starts -- exactly back-to-back pair steps of pass_batch samples (left to the per-tower calls, the faster tower runs a
            # whole pass ahead and a bs = 512 step measured 5 % SLOWER than one pass; profiles/r06_batch_scaling.txt).  Same bits.
            k = -(-n // self.pass_batch)
            bounds = [(i * n // k, (i + 1) * n // k) for i in range(k)]
            parts = [self._encode_pair_two_streams(pixels[a:b], input_ids[a:b], None if attention_mask is None else attention_mask[a:b],
                                                   normalize) for a, b in bounds]
            return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
        if not overlap:
            return self._encode_image_any(pixels, normalize), self.encode_text(input_ids, attention_mask, normalize)
        return self._encode_pair_two_streams(pixels, input_ids, attention_mask, normalize)

    def _encode_image_any(self, pixels: torch.Tensor, normalize: bool):
        """fp32 NCHW pixels or native uint8 [B,H,W,3] tiles (normalisation fused on the GPU) -- the two image inputs of the path"""
        return self.encode_image_u8(pixels, normalize) if pixels.dtype == torch.uint8 else self.encode_image(pixels, normalize)

    def _encode_pair_two_streams(self, pixels, input_ids, attention_mask, normalize):
        main = torch.cuda.current_stream(self.device)
        # ONE side stream per (device, caller's stream) and process, shared by every engine, picked once by MEASURING that it runs beside
        # the caller's (pair_stream): which hardware queue a new stream lands on depends on how many streams the process created before,
        # and two towers on one queue run in order -- 4.47 instead of 4.28 ms per step (profiles/r06_batch_scaling.txt).
        side = self.pair_stream(main)
        side.wait_stream(main)                      # inputs produced on the main stream are ready
        with torch.cuda.stream(side):
            txt = self.encode_text(input_ids, attention_mask, normalize)
        if self.pair_vision_priority:
            # experiment (tools/gpu_diag.py prio): the longer tower on a high-priority stream of its own, the shorter one
            # filling the gaps -- see profiles/r02_two_stream_priority.txt for what it measured
            if self._vis is None:
                self._vis = torch.cuda.Stream(device=self.device, priority=-1)
            self._vis.wait_stream(main)
            with torch.cuda.stream(self._vis):
                img = self._encode_image_any(pixels, normalize)
            main.wait_stream(self._vis)
            img.record_stream(main)
        else:
            img = self._encode_image_any(pixels, normalize)
        main.wait_stream(side)
        txt.record_stream(main)
        return img, txt
