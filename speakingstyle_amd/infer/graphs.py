"""HIP-graph synthesis for small batches (serving latency; reference ``synthesize.py:128-150`` single mode, the
batch-1 path of ``notebooks/control.ipynb:778``).

A batch-1 text -> wav synthesis is ~350 kernel launches driven from Python: ~3 ms of host time against well under
1 ms of GPU work, so the latency is the host's.  Here the packed synthesis path (``FastSpeech2.infer_front`` /
``infer_back`` + ``Generator.infer_packed``) is captured in two HIP graphs and replayed:

  * graph 1: style encoder, encoder, variance adaptor, duration rounding -> the mel lengths (device);
  * the one host sync of any FastSpeech2 synthesis: the B mel lengths come back to the host;
  * graph 2: packed length regulator + decoder, mel_linear, PostNet and the packed HiFi-GAN down to the int16
    waveform.

Every replay recomputes the whole text -> wav path from its inputs (copied into the graph's static input
tensors first); only launch overhead is removed.  A key is captured after ``warm`` eager runs on it (allocations,
workspaces, the vocoder's length tables settle); keys seen for the first time run eagerly.

Exact keys (the default): graph 1 per (B, text length, reference-mel shape, controls), graph 2 per (graph-1 entry,
tuple of mel lengths).  Right for a caller that repeats utterances; a stream of distinct utterances almost never
repeats a length tuple and stays eager.

Bucketed (``bucketed=True``): one graph serves every utterance that fits its bucket.  Graph 1 runs B + 1 rows of
``Tb`` phonemes (the text length rounded up to 16; ``FastSpeech2.pad_for_bucket``): the real rows padded with the pad
id, and a one-phoneme filler row.  After the D2H of the lengths the host only picks a capacity (``hip.cap_bucket``:
Rcap rows >= sum(lens) + 1, Mcap frames) and graph 2, keyed (graph-1 entry, Rcap, Mcap), runs at R = Rcap, M = Mcap
with B + 1 sequences: its first node (``hip.VocPackCap.update``) reads the real lengths on the device, gives the
filler the F = Rcap - sum(lens) rows left over and writes every vocoder table, padded with null tiles.  The packed
kernels keep sequences from touching each other, so the real rows come out as they would alone; the caller gets the
first B rows of the [B + 1, Mcap * hop] buffer, cut to max(lens) * hop samples.

Lifetimes: a captured graph keeps its memory (the shared pool) and every kernel workspace it captured
(``hip._GRAPHS_LIVE``: grown workspaces are retired, never freed).  A graph-2 entry holds its graph-1 entry (whose
static outputs it reads) and the vocoder pack whose tables it reads (``VocPack`` / ``VocPackCap``; the kernel
library's own LRU of packs is smaller than ``max_graphs``).  The graphs read the bf16 weight images in place:
the weight generation (``hip.bump_weight_generation``) is recorded at capture and every graph is dropped when it
has moved on.
"""
from __future__ import annotations

import collections
import time

import torch

from ..ops import weights


def _multi_copy(pairs) -> bool:
    from ..ops import hip

    return hip.multi_copy(pairs)


def _ctl_key(c):
    return ("t", tuple(c.shape)) if isinstance(c, torch.Tensor) else float(c)


class SynthGraphs:
    def __init__(self, model, vocoder, int16_scale=None, warm: int = 1, max_batch: int = 8, max_graphs: int = 64,
                 bucketed: bool = False):
        self.model, self.voc = model, vocoder
        self.scale = int16_scale
        self.warm, self.max_batch, self.max_graphs = int(warm), int(max_batch), int(max_graphs)
        self.bucketed = bool(bucketed)
        self.g1 = collections.OrderedDict()
        self.g2 = collections.OrderedDict()
        self.packs = {}  # bucketed: (B, Rcap, Mcap, device) -> VocPackCap (static tables, rewritten by every run)
        self.pool = None
        self.stream = None  # warm-up AND capture run on this one stream: the stream-keyed workspaces of the kernel
        #                     library (split-K partials) are allocated by the warm-up, never inside a capture
        self.wgen = None  # weight generation the live graphs were captured at
        self.stats = {"captures": 0, "replays": 0, "eager": 0, "capture_s": 0.0}

    def supported(self, texts) -> bool:
        return (texts.is_cuda and texts.shape[0] <= self.max_batch and self.model.packed_inference_ok(texts)
                and self.voc.packable())

    # ------------------------------------------------------------------ eager halves
    def _front(self, inp, padded=False):
        """``padded``: inp are ``pad_for_bucket`` rows -- each must come out as its unpadded text would."""
        return self.model.infer_front(*inp, exact_pad=padded)

    def _back(self, front, lens):
        rows = self.model.infer_back(front, lens)
        return self.voc.infer_packed(rows, lens, int16_scale=self.scale)

    def _back_cap(self, front, pack):
        """The bucketed second half: size the filler and write the tables on the device, then run at capacity
        -> [B + 1, Mcap * hop]."""
        pack.update(front[2], front[1])
        rows = self.model.infer_back(front, None, cap=(pack.R, pack.M))
        return self.voc.infer_packed(rows, None, int16_scale=self.scale, cap=pack)

    def _pack(self, B, lens, device):
        from ..ops import hip

        rcap, mcap = hip.cap_bucket(lens)
        key = (B, rcap, mcap, str(device))
        pack = self.packs.get(key)
        if pack is None:
            pack = self.packs[key] = self.voc.cap_pack(B, rcap, mcap, device)
        return key, pack

    @staticmethod
    def _crop_m(out, lens, pack):
        """The caller's [B, max(lens) * hop] wav (a fresh tensor) of a capacity result; the filler row is dropped."""
        hop = out.shape[1] // pack.M
        return out[: len(lens), : max(lens) * hop].clone()

    def _pad(self, inp):
        speakers, texts, src_lens, _, mels, mel_lens, max_mel_len, pc, ec, dc, sw = inp
        Tb = self.model.pad_text_bucket(texts.shape[1])
        sp, tp, sl, mp, mlp, swp, (pc, ec, dc) = self.model.pad_for_bucket(speakers, texts, src_lens, Tb, mels,
                                                                          mel_lens, sw, (pc, ec, dc))
        return (sp, tp, sl, Tb, mp, mlp, max_mel_len, pc, ec, dc, swp)

    # ------------------------------------------------------------------ capture helpers
    def _capture(self, fn):
        from ..ops import hip

        hip.graphs_live()  # grown workspaces are retired from now on (graphs hold their addresses)
        if self.pool is None:
            self.pool = torch.cuda.graph_pool_handle()
        t0 = time.perf_counter()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, pool=self.pool, stream=self.stream):
            out = fn()
        torch.cuda.synchronize()
        self.wgen = weights.generation()
        self.stats["captures"] += 1
        self.stats["capture_s"] += time.perf_counter() - t0
        return g, out

    def _evict(self, table):
        while len(table) > self.max_graphs:
            table.popitem(last=False)

    def _check_weights(self):
        """The graphs replay kernels on the weight images they were captured with: drop them all once the weights
        have been declared changed (``hip.bump_weight_generation``); the next calls warm and capture again."""
        if self.wgen is not None and self.wgen != weights.generation():
            torch.cuda.synchronize()
            self.g2.clear()
            self.g1.clear()
            self.pool = None  # the allocator frees a graph pool with its last graph: the next capture opens a new one
            self.wgen = None

    def _entry(self, table, key, **extra):
        e = table.get(key)
        if e is None:
            e = table[key] = {"seen": 0, "graph": None, **extra}
            self._evict(table)
        else:
            table.move_to_end(key)
        return e

    # ------------------------------------------------------------------ synthesis
    @torch.no_grad()
    def __call__(self, speakers, texts, src_lens, max_src_len, mels=None, mel_lens=None, max_mel_len=None,
                 p_control=1.0, e_control=1.0, d_control=1.0, style_weights=None):
        """-> (wav [B, max(lens) * hop] (int16 when int16_scale), host mel lengths).  The wav is a fresh tensor,
        ordered on the caller's stream."""
        return self._on_stream(texts, self._run, speakers, texts, src_lens, max_src_len, mels, mel_lens, max_mel_len,
                               p_control, e_control, d_control, style_weights)

    @torch.no_grad()
    def eager(self, speakers, texts, src_lens, max_src_len, mels=None, mel_lens=None, max_mel_len=None,
              p_control=1.0, e_control=1.0, d_control=1.0, style_weights=None):
        """The same composition as ``__call__`` launched kernel by kernel, touching no graph and no counter (what a
        replay must reproduce bit for bit)."""
        return self._on_stream(texts, self._eager, speakers, texts, src_lens, max_src_len, mels, mel_lens,
                               max_mel_len, p_control, e_control, d_control, style_weights)

    def _on_stream(self, texts, fn, *args):
        if not texts.is_cuda:
            return fn(*args)
        if self.stream is None:
            self.stream = torch.cuda.Stream(device=texts.device)
        cur = torch.cuda.current_stream(texts.device)
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            wav, lens = fn(*args)
        cur.wait_stream(self.stream)
        wav.record_stream(cur)
        return wav, lens

    @staticmethod
    def _inp(speakers, texts, src_lens, max_src_len, mels, mel_lens, max_mel_len, pc, ec, dc, sw):
        return (speakers, texts, src_lens, int(max_src_len), mels, mel_lens,
                None if max_mel_len is None else int(max_mel_len), pc, ec, dc, sw)

    def _eager(self, *args):
        inp = self._inp(*args)
        texts = inp[1]
        if self.bucketed and self.supported(texts):
            B = texts.shape[0]
            front = self._front(self._pad(inp), True)
            lens = [int(v) for v in front[2][:B].cpu().tolist()]
            _, pack = self._pack(B, lens, texts.device)
            return self._crop_m(self._back_cap(front, pack), lens, pack), lens
        front = self._front(inp)
        lens = [int(v) for v in front[2].cpu().tolist()]
        return self._back(front, lens), lens

    def _run(self, *args):
        inp = self._inp(*args)
        texts, mels, sw = inp[1], inp[4], inp[10]
        if not self.supported(texts):
            self.stats["eager"] += 1
            return self._eager(*args)
        self._check_weights()
        B = texts.shape[0]
        if self.bucketed:
            inp = self._pad(inp)
        # (bucketed: inp[1] is the padded [B + 1, Tb] text, so the shape key is the bucket)
        k1 = (tuple(inp[1].shape), None if mels is None else tuple(mels.shape), inp[3], inp[6],
              tuple(_ctl_key(c) for c in inp[7:10]), None if sw is None else tuple(sw.shape), str(texts.device))
        e1 = self._entry(self.g1, k1)
        if e1["graph"] is None:
            if e1["seen"] < self.warm:
                e1["seen"] += 1
                self.stats["eager"] += 1
                return self._eager(*args)
            static = tuple(t.clone() if isinstance(t, torch.Tensor) else t for t in inp)
            e1["static"] = static
            e1["graph"], e1["out"] = self._capture(lambda: self._front(static, self.bucketed))
        # every static input is overwritten whole (bucketed: the padded rows, so no tail of a longer text survives)
        pairs = [(dst, src) for dst, src in zip(e1["static"], inp) if isinstance(dst, torch.Tensor)]
        if not _multi_copy(pairs):  # one launch for all inputs when they are device tensors
            for dst, src in pairs:
                dst.copy_(src, non_blocking=True)
        e1["graph"].replay()
        self.stats["replays"] += 1
        lens = [int(v) for v in e1["out"][2].cpu().tolist()][:B]  # the one host sync (bucketed: not the filler's)
        # graph 2 reads THIS graph-1 entry's static outputs: keyed by the entry object (held by the graph-2 entry,
        # so its id stays unique while the entry lives), not by the shape key
        if self.bucketed:
            pk, pack = self._pack(B, lens, texts.device)
            e2 = self._entry(self.g2, (id(e1),) + pk[1:3], front=e1, pack=pack)

            def back():
                return self._back_cap(e1["out"], pack)

            def result(out):
                return self._crop_m(out, lens, pack)
        else:
            e2 = self._entry(self.g2, (id(e1), tuple(lens)), front=e1)

            def back():
                return self._back(e1["out"], lens)

            def result(out):
                return out.clone()
        if e2["graph"] is None:
            if e2["seen"] < self.warm:
                e2["seen"] += 1
                self.stats["eager"] += 1
                return result(back()), lens
            if not self.bucketed:
                # the tables the capture will read: the entry keeps them (the library's LRU alone would let them go
                # while this graph lives)
                from ..ops import hip

                e2["pack"] = hip.voc_pack_for(lens, texts.device, self.voc._packed_geoms(lens))
            e2["graph"], e2["out"] = self._capture(back)
        e2["graph"].replay()
        self.stats["replays"] += 1
        return result(e2["out"]), lens
