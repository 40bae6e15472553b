"""Speaker clustering and diarized text over the C ABI (crispy_diar_*, include/crispy_hip.h): the reference's `nme_sc`, the
tail of `run_diarization` and `format_diarized_text` (src-tauri/src/managers/diarization.rs:276-724).  Embeddings are the
caller's; there is no CPU path for the clustering.  The host functions (`chunk_plan`, `speaker_segments`, `find_speaker`,
`format_diarized_text`) need no device.

The front end (crispy_diar_fbank*, crispy_diar_speech_segments): `segmentation_windows`, `speech_segments`, `Diarizer.fbank`
and `run_diarization`, which is the reference's run_diarization (:276-409) with its two networks as callables.

The segmentation network (crispy_diar_seg_*): `Diarizer.load_segmentation`, `seg_forward`, `segmentation_scores[_device]`,
`seg_frames`, `seg_windows`; with it loaded, `run_diarization(pcm, None, emb_fn, ...)` needs the embedding network alone.

The embedding network (crispy_diar_emb_*, crispy_diar_embed*): `Diarizer.load_embedding`, `embed`, `embed_chunks[_device]`,
`emb_frames`, `emb_tensor_spec`; with both loaded, `run_diarization(pcm, None, None, ...)` needs no callable at all."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a, ty):
    return a.ctypes.data_as(C.POINTER(ty)) if a.size else None


class Diarizer:
    """A crispy_diar handle: its own stream and a scratch that grows on demand."""

    def __init__(self, device: int = 0, lib=None):
        self._L = lib or N.lib()
        self._h = C.c_void_p()
        N.check(self._L.crispy_diar_create(int(device), C.byref(self._h)), self._L)

    def close(self):
        if self._h:
            self._L.crispy_diar_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def cluster(self, recordings, max_speakers: int):
        """nme_sc for a list of [n_i, dim] f32 arrays in one call -> (list of int32 label arrays, list of info dicts)."""
        recs = [np.ascontiguousarray(r, dtype=np.float32) for r in recordings]
        dim = recs[0].shape[1]
        n = np.array([r.shape[0] for r in recs], np.int32)
        emb = np.ascontiguousarray(np.concatenate([r.reshape(-1, dim) for r in recs], 0))
        labels = np.zeros(int(n.sum()), np.int32)
        info = (N.DiarInfo * len(recs))()
        N.check(self._L.crispy_diar_cluster(self._h, emb.ctypes.data, _p(n, C.c_int), len(recs), dim, int(max_speakers),
                                            labels.ctypes.data, C.cast(info, C.c_void_p)), self._L)
        off = np.concatenate([[0], np.cumsum(n)])
        return ([labels[off[i]:off[i + 1]].copy() for i in range(len(recs))],
                [dict(p_star=x.p_star, k=x.k, ratio=x.ratio, gap=x.gap, p_max=x.p_max) for x in info])

    def cluster_device(self, emb, n, max_speakers: int, stream=None):
        """The same on a CUDA f32 tensor [sum n, dim] -> (int32 CUDA tensor [sum n], DiarInfo array)."""
        import torch
        n = np.ascontiguousarray(n, dtype=np.int32)
        labels = torch.zeros(int(n.sum()), dtype=torch.int32, device=emb.device)
        info = (N.DiarInfo * len(n))()
        N.check(self._L.crispy_diar_cluster_device(self._h, emb.data_ptr(), _p(n, C.c_int), len(n), emb.shape[1], int(max_speakers),
                                                   labels.data_ptr(), C.cast(info, C.c_void_p), stream), self._L)
        return labels, info

    def affinity(self, emb):
        import torch
        out = torch.empty((emb.shape[0], emb.shape[0]), dtype=torch.float32, device=emb.device)
        N.check(self._L.crispy_diar_affinity_device(self._h, emb.data_ptr(), emb.shape[0], emb.shape[1], out.data_ptr()), self._L)
        return out

    def laplacian(self, aff, p: int):
        import torch
        out = torch.empty_like(aff)
        N.check(self._L.crispy_diar_laplacian_device(self._h, aff.data_ptr(), aff.shape[0], int(p), out.data_ptr()), self._L)
        return out

    def eigh(self, mats, vectors: bool = True):
        """mats: CUDA f32 [n_mats, n, n] symmetric -> (evals [n_mats, n] ascending, evecs [n_mats, n, n] or None)."""
        import torch
        m, n = mats.shape[0], mats.shape[1]
        ev = torch.empty((m, n), dtype=torch.float32, device=mats.device)
        vec = torch.empty((m, n, n), dtype=torch.float32, device=mats.device) if vectors else None
        N.check(self._L.crispy_diar_eigh_device(self._h, mats.data_ptr(), n, m, ev.data_ptr(), vec.data_ptr() if vectors else None), self._L)
        return ev, vec

    def decide(self, evals, n: int, max_speakers: int) -> dict:
        """The eigengap decision alone.  evals: CUDA f32 [p_max, n], row p - 1 ascending, or None -> info dict."""
        p_max = 0 if evals is None else evals.shape[0]
        info = N.DiarInfo()
        N.check(self._L.crispy_diar_decide_device(self._h, evals.data_ptr() if p_max and n else None, int(n), p_max, int(max_speakers),
                                                  C.cast(C.pointer(info), C.c_void_p)), self._L)
        return dict(p_star=info.p_star, k=info.k, ratio=info.ratio, gap=info.gap, p_max=info.p_max)

    def kmeans(self, vecs, k: int, details: bool = False):
        """Spectral rows and k-means alone.  vecs: CUDA f32 [n, n] (the first k columns are read) -> int32 CUDA labels [n],
        with `details` also the normalised points [n, k] and the final centres [k, k] (None where k <= 1 or k >= n)."""
        import torch
        n = vecs.shape[0]
        labels = torch.zeros(n, dtype=torch.int32, device=vecs.device)
        pts = ctr = None
        if details and 1 < k < n:
            pts = torch.zeros((n, k), dtype=torch.float32, device=vecs.device)
            ctr = torch.zeros((k, k), dtype=torch.float32, device=vecs.device)
        N.check(self._L.crispy_diar_kmeans_device(self._h, vecs.data_ptr() if n else None, n, int(k), labels.data_ptr() if n else None,
                                                  pts.data_ptr() if pts is not None else None,
                                                  ctr.data_ptr() if ctr is not None else None), self._L)
        return (labels, pts, ctr) if details else labels

    def fbank(self, pcm, chunks, scale: float = 1.0):
        """The embedding network's features (EmbeddingExtractor::compute, :53-75).  pcm: 16 kHz mono numpy int16 or float32
        (f32 goes through f32_to_i16 on the device); chunks: (first sample, n samples) pairs -> list of f32 [frames, 80] arrays,
        one per chunk (no rows for a chunk of fewer than 400 samples)."""
        pcm = np.ascontiguousarray(pcm)
        fmt = _pcm_format(pcm.dtype)
        first, ln, off = _chunk_arrays(chunks)
        args = (self._h, pcm.ctypes.data if pcm.size else None, fmt, _p(first, C.c_long), _p(ln, C.c_long), len(first), float(scale))
        N.check(self._L.crispy_diar_fbank(*args, None, _p(off, C.c_long)), self._L)
        feats = np.zeros((int(off[-1]), N.FBANK_BINS), np.float32)
        if feats.size:
            N.check(self._L.crispy_diar_fbank(*args, feats.ctypes.data, _p(off, C.c_long)), self._L)
        return [feats[off[c]:off[c + 1]] for c in range(len(first))]

    def fbank_device(self, pcm, chunks, scale: float = 1.0, raw: bool = False, stream=None):
        """The same on a CUDA int16 or float32 tensor -> (f32 CUDA tensor [rows, 80], frame_offset int64 [n_chunks + 1]), with
        `raw` also the rows before the mean subtraction."""
        import torch
        fmt = _pcm_format(pcm.dtype)
        first, ln, off = _chunk_arrays(chunks)
        args = (self._h, pcm.data_ptr() if pcm.numel() else None, fmt, _p(first, C.c_long), _p(ln, C.c_long), len(first), float(scale))
        N.check(self._L.crispy_diar_fbank_device(*args, None, None, _p(off, C.c_long), stream), self._L)
        feats = torch.empty((int(off[-1]), N.FBANK_BINS), dtype=torch.float32, device=pcm.device)
        rows = torch.empty_like(feats) if raw else None
        if feats.numel():
            if stream is None:      # the handle's stream does not wait for torch's: what produced pcm must have finished
                torch.cuda.current_stream(pcm.device).synchronize()
            N.check(self._L.crispy_diar_fbank_device(*args, feats.data_ptr(), rows.data_ptr() if raw else None, _p(off, C.c_long), stream),
                    self._L)
        return (feats, rows, off) if raw else (feats, off)

    # ---- the segmentation network (crispy_diar_seg_*) ----
    def load_segmentation(self, tensors: dict):
        """The weights of pyannote segmentation-3.0 by their state-dict keys (`sincnet.conv1d.0.filters` is the evaluated
        [80, 1, 251] sinc bank): name -> array-like, taken as f32.  A second load replaces the first."""
        arrs = [np.ascontiguousarray(np.asarray(v, dtype=np.float32)).reshape(-1) for v in tensors.values()]
        n = len(arrs)
        names = (C.c_char_p * max(n, 1))(*[str(k).encode("utf-8") for k in tensors])
        data = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in arrs])
        count = np.ascontiguousarray([a.size for a in arrs], dtype=np.int64)
        N.check(self._L.crispy_diar_seg_load(self._h, names, data, _p(count, C.c_long), n), self._L)

    @property
    def segmentation_loaded(self) -> bool:
        return bool(self._L.crispy_diar_seg_loaded(self._h))

    def seg_forward(self, windows, taps: bool = False, stream=None):
        """The network on windows of one length: f32 [n_win, len] (numpy or CUDA tensor), 991 <= len <= 160000 ->
        scores [n_win, frames, 7]; with `taps` also the SincNet output [n_win, frames, 60] and the last LSTM layer's
        [n_win, frames, 256].  numpy in gives numpy out, a CUDA tensor gives CUDA tensors."""
        import torch
        host = not isinstance(windows, torch.Tensor)
        x = torch.from_numpy(np.ascontiguousarray(windows, dtype=np.float32)).cuda() if host else windows.contiguous()
        if x.dim() != 2 or x.dtype != torch.float32:
            raise ValueError("windows must be f32 [n_win, len]")
        n_win, ln = int(x.shape[0]), int(x.shape[1])
        fr = seg_frames(ln)
        scores = torch.empty((n_win, fr, N.SEG_CLASSES), dtype=torch.float32, device=x.device)
        sinc = torch.empty((n_win, fr, 60), dtype=torch.float32, device=x.device) if taps else None
        lstm = torch.empty((n_win, fr, 256), dtype=torch.float32, device=x.device) if taps else None
        if stream is None:      # the handle's stream does not wait for torch's
            torch.cuda.current_stream(x.device).synchronize()
        N.check(self._L.crispy_diar_seg_forward_device(self._h, x.data_ptr() if x.numel() else None, n_win, ln, scores.data_ptr() if fr else None,
                                                       sinc.data_ptr() if taps else None, lstm.data_ptr() if taps else None, stream), self._L)
        out = (scores, sinc, lstm) if taps else (scores,)
        if host:
            out = tuple(o.cpu().numpy() for o in out)
        return out if taps else out[0]

    def segmentation_scores(self, pcm) -> np.ndarray:
        """pyannote_get_segments_fixed up to the network's output (:103-145) for a whole recording.  pcm: 16 kHz mono numpy
        int16 or float32 (f32 goes through f32_to_i16 on the device) -> f32 [n_windows, 589, 7], what speech_segments takes."""
        pcm = np.ascontiguousarray(pcm)
        fmt = _pcm_format(pcm.dtype)
        scores = np.zeros((seg_windows(pcm.size), N.SEG_FRAMES, N.SEG_CLASSES), np.float32)
        N.check(self._L.crispy_diar_seg_scores(self._h, pcm.ctypes.data if pcm.size else None, fmt, pcm.size,
                                               scores.ctypes.data if scores.size else None), self._L)
        return scores

    def segmentation_scores_device(self, pcm, stream=None):
        """The same on a CUDA int16 or float32 tensor -> f32 CUDA tensor [n_windows, 589, 7]."""
        import torch
        fmt = _pcm_format(pcm.dtype)
        n = int(pcm.numel())
        scores = torch.empty((seg_windows(n), N.SEG_FRAMES, N.SEG_CLASSES), dtype=torch.float32, device=pcm.device)
        if stream is None:
            torch.cuda.current_stream(pcm.device).synchronize()
        N.check(self._L.crispy_diar_seg_scores_device(self._h, pcm.data_ptr() if n else None, fmt, n,
                                                      scores.data_ptr() if scores.numel() else None, stream), self._L)
        return scores

    # ---- the embedding network (crispy_diar_emb_*) ----
    def load_embedding(self, tensors: dict):
        """The weights of WeSpeaker CAMPPlus by their state-dict keys: name -> array-like, taken as f32 (`*.num_batches_tracked`
        entries are dropped, so a torch state dict goes in as it is).  A second load replaces the first."""
        items = [(str(k), v) for k, v in tensors.items() if not str(k).endswith("num_batches_tracked")]
        arrs = [np.ascontiguousarray(np.asarray(v, dtype=np.float32)).reshape(-1) for _k, v in items]
        n = len(arrs)
        names = (C.c_char_p * max(n, 1))(*[k.encode("utf-8") for k, _v in items])
        data = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in arrs])
        count = np.ascontiguousarray([a.size for a in arrs], dtype=np.int64)
        N.check(self._L.crispy_diar_emb_load(self._h, names, data, _p(count, C.c_long), n), self._L)

    @property
    def embedding_loaded(self) -> bool:
        return bool(self._L.crispy_diar_emb_loaded(self._h))

    @property
    def embedding_dim(self) -> int:
        return int(self._L.crispy_diar_emb_dim(self._h))

    def embed(self, feats_list, taps: bool = False, stream=None):
        """The network on a list of chunks, each f32 [rows, 80] with 3 <= rows <= 30000 (numpy arrays or CUDA tensors), in one
        call -> embeddings [n_chunks, dim]; with `taps` also the head's output (a list of [rows, 320]), the rows in front of the
        pooling (a list of [emb_frames(rows), 512]) and the statistics [n_chunks, 1024].  numpy in gives numpy out, CUDA tensors
        give CUDA tensors."""
        import torch
        host = not (len(feats_list) and isinstance(feats_list[0], torch.Tensor))
        if host:
            rows = [np.ascontiguousarray(f, dtype=np.float32).reshape(-1, N.FBANK_BINS) for f in feats_list]
            x = torch.from_numpy(np.concatenate(rows, 0) if rows else np.zeros((0, N.FBANK_BINS), np.float32)).cuda()
        else:
            rows = [f.reshape(-1, N.FBANK_BINS) for f in feats_list]
            x = torch.cat(rows, 0).contiguous()
            if x.dtype != torch.float32:
                raise ValueError("features must be f32 [rows, 80]")
        n = len(rows)
        off = np.zeros(n + 1, np.int64)
        off[1:] = np.cumsum([int(r.shape[0]) for r in rows])
        t2 = [emb_frames(int(r.shape[0])) for r in rows]
        dim = self.embedding_dim
        emb = torch.empty((n, dim), dtype=torch.float32, device=x.device)
        head = torch.empty((int(off[-1]), N.EMB_HEAD), dtype=torch.float32, device=x.device) if taps else None
        xvec = torch.empty((sum(t2), N.EMB_XVEC), dtype=torch.float32, device=x.device) if taps else None
        stats = torch.empty((n, N.EMB_STATS), dtype=torch.float32, device=x.device) if taps else None
        if stream is None:      # the handle's stream does not wait for torch's
            torch.cuda.current_stream(x.device).synchronize()
        N.check(self._L.crispy_diar_emb_forward_device(self._h, x.data_ptr() if x.numel() else None, _p(off, C.c_long), n,
                                                       emb.data_ptr() if emb.numel() else None, head.data_ptr() if taps else None,
                                                       xvec.data_ptr() if taps else None, stats.data_ptr() if taps else None, stream), self._L)
        if not taps:
            return emb.cpu().numpy() if host else emb
        q = np.concatenate([[0], np.cumsum(t2)])
        heads = [head[off[c]:off[c + 1]] for c in range(n)]
        xvecs = [xvec[q[c]:q[c + 1]] for c in range(n)]
        if host:
            return emb.cpu().numpy(), [t.cpu().numpy() for t in heads], [t.cpu().numpy() for t in xvecs], stats.cpu().numpy()
        return emb, heads, xvecs, stats

    def embed_chunks(self, pcm, chunks, scale: float = 1.0) -> np.ndarray:
        """EmbeddingExtractor::compute (:53-75) for all chunks of a recording in one call.  pcm: 16 kHz mono numpy int16 or float32
        (f32 goes through f32_to_i16 on the device); chunks: (first sample, n samples) pairs, each of at least 3 feature rows
        (fbank_frames) -> f32 [n_chunks, dim].  The feature rows stay on the device."""
        pcm = np.ascontiguousarray(pcm)
        fmt = _pcm_format(pcm.dtype)
        first, ln, _off = _chunk_arrays(chunks)
        emb = np.zeros((len(first), self.embedding_dim), np.float32)
        N.check(self._L.crispy_diar_embed(self._h, pcm.ctypes.data if pcm.size else None, fmt, _p(first, C.c_long), _p(ln, C.c_long), len(first),
                                          float(scale), emb.ctypes.data if emb.size else None), self._L)
        return emb

    def embed_chunks_device(self, pcm, chunks, scale: float = 1.0, stream=None):
        """The same on a CUDA int16 or float32 tensor -> f32 CUDA tensor [n_chunks, dim]."""
        import torch
        fmt = _pcm_format(pcm.dtype)
        first, ln, _off = _chunk_arrays(chunks)
        emb = torch.empty((len(first), self.embedding_dim), dtype=torch.float32, device=pcm.device)
        if stream is None:
            torch.cuda.current_stream(pcm.device).synchronize()
        N.check(self._L.crispy_diar_embed_device(self._h, pcm.data_ptr() if pcm.numel() else None, fmt, _p(first, C.c_long), _p(ln, C.c_long),
                                                 len(first), float(scale), emb.data_ptr() if emb.numel() else None, stream), self._L)
        return emb


def _pcm_format(dtype) -> int:
    name = str(dtype).replace("torch.", "")
    if name == "int16":
        return N.PCM_I16
    if name == "float32":
        return N.PCM_F32
    raise TypeError(f"pcm must be int16 or float32, not {dtype}")


def _chunk_arrays(chunks):
    first = np.ascontiguousarray([c[0] for c in chunks], dtype=np.int64)
    ln = np.ascontiguousarray([c[1] for c in chunks], dtype=np.int64)
    return first, ln, np.zeros(len(first) + 1, np.int64)


def fbank_frames(n: int) -> int:
    """Rows of the fbank for n samples (snip_edges: 400 samples at hop 160)."""
    return int(N.lib().crispy_diar_fbank_frames(int(n)))


def f32_to_i16(x) -> np.ndarray:
    """f32_to_i16 (:649-654): (s.clamp(-1, 1) * 32767.0) as i16 -- truncating, NaN -> 0."""
    x = np.asarray(x, np.float32)
    v = np.clip(x, np.float32(-1), np.float32(1)) * np.float32(32767.0)
    return np.where(np.isnan(v), np.float32(0), v).astype(np.int16)


SEG_WINDOW = 160000      # the segmentation network's 10 s window


def segmentation_windows(pcm_i16) -> np.ndarray:
    """The network inputs of pyannote_get_segments_fixed (:103-128): the samples padded with zeros to a multiple of 10 s plus
    one more window, as i16 / 32768 -> f32 [n_windows, 160000] (no window for no samples)."""
    x = np.ascontiguousarray(pcm_i16, dtype=np.int16)
    if x.size == 0:
        return np.zeros((0, SEG_WINDOW), np.float32)
    n_win = -(-x.size // SEG_WINDOW) + 1
    out = np.zeros(n_win * SEG_WINDOW, np.float32)
    out[:x.size] = x.astype(np.float32) / np.float32(32768.0)
    return out.reshape(n_win, SEG_WINDOW)


def speech_segments(scores, n_samples: int, merge_gap: float, sample_rate: int = 16000):
    """The post-network half of pyannote_get_segments_fixed (:146-271).  scores: f32 [n_windows, n_frames, n_classes] ->
    list of (start s, end s, first sample, n samples)."""
    L = N.lib()
    sc = np.ascontiguousarray(scores, dtype=np.float32)
    if sc.ndim != 3:
        raise ValueError("scores must be [n_windows, n_frames, n_classes]")
    args = (sc.ctypes.data if sc.size else None, sc.shape[0], sc.shape[1], sc.shape[2], int(n_samples), int(sample_rate), float(merge_gap))
    cnt = L.crispy_diar_speech_segments(*args, None, None, None, None, 0)
    if cnt < 0:
        N.check(int(cnt), L)
    os_, oe = np.zeros(cnt), np.zeros(cnt)
    of, ol = np.zeros(cnt, np.int64), np.zeros(cnt, np.int64)
    if cnt:
        L.crispy_diar_speech_segments(*args, _p(os_, C.c_double), _p(oe, C.c_double), _p(of, C.c_long), _p(ol, C.c_long), cnt)
    return [(float(os_[i]), float(oe[i]), int(of[i]), int(ol[i])) for i in range(cnt)]


def seg_frames(n: int) -> int:
    """Frames the segmentation network gives for a window of n samples (589 at 160000, 0 below 991)."""
    return int(N.lib().crispy_diar_seg_frames(int(n)))


def seg_windows(n: int) -> int:
    """Windows of a recording of n samples: 0 for 0, else ceil(n / 160000) + 1."""
    return int(N.lib().crispy_diar_seg_windows(int(n)))


def emb_frames(rows: int) -> int:
    """Positions the embedding network keeps of `rows` feature rows after its stride-2 layer: (rows - 1) // 2 + 1, 0 without rows."""
    return int(N.lib().crispy_diar_emb_frames(int(rows)))


def emb_tensor_spec(dim: int = 512):
    """The tensors Diarizer.load_embedding expects for an embedding width `dim`: [(state-dict key, element count)]."""
    L = N.lib()
    name, count = C.c_char_p(), C.c_long()
    n = L.crispy_diar_emb_tensor_spec(0, int(dim), None, None)
    N.check(min(n, 0), L)
    out = []
    for i in range(n):
        N.check(min(L.crispy_diar_emb_tensor_spec(i, int(dim), C.byref(name), C.byref(count)), 0), L)
        out.append((name.value.decode("utf-8"), int(count.value)))
    return out


def run_diarization(pcm, seg_fn, emb_fn, max_speakers: int, merge_gap: float, diarizer: "Diarizer"):
    """run_diarization (:276-409).  pcm: 16 kHz mono, f32 in [-1, 1] (taken through f32_to_i16) or int16;
    seg_fn(window f32 [160000]) -> [frames, classes], or None for the network loaded into `diarizer`
    (Diarizer.load_segmentation); emb_fn(features f32 [frames, 80]) -> [dim], or None for the network loaded into `diarizer`
    (Diarizer.load_embedding: all chunks in one call, the features staying on the device; a chunk of fewer than 3 feature rows
    is dropped like one without rows).  -> merged [(start, end, speaker number >= 1)]."""
    pcm = np.asarray(pcm)
    x = pcm if pcm.dtype == np.int16 else f32_to_i16(pcm)
    if seg_fn is None and not diarizer.segmentation_loaded:
        raise ValueError("run_diarization: seg_fn is None and no segmentation network is loaded (Diarizer.load_segmentation)")
    if emb_fn is None and not diarizer.embedding_loaded:
        raise ValueError("run_diarization: emb_fn is None and no embedding network is loaded (Diarizer.load_embedding)")
    if x.size == 0:
        return []
    if seg_fn is None:
        scores = diarizer.segmentation_scores(x)
    else:
        scores = np.stack([np.asarray(seg_fn(w), np.float32) for w in segmentation_windows(x)])
    segments = speech_segments(scores, x.size, merge_gap)
    if not segments:
        return []
    plan = chunk_plan([(s, e, n) for s, e, _first, n in segments])
    if emb_fn is None:
        keep = [c for c in range(len(plan)) if fbank_frames(plan[c][4]) >= N.EMB_MIN_ROWS]
        if not keep:
            return []
        emb = diarizer.embed_chunks(x, [(segments[plan[c][2]][2] + plan[c][3], plan[c][4]) for c in keep])
        labels = diarizer.cluster([emb], max(int(max_speakers), 1))[0][0]
        return speaker_segments([plan[c][0] for c in keep], [plan[c][1] for c in keep], labels, merge_gap)
    feats = diarizer.fbank(x, [(segments[seg][2] + first, n) for _s, _e, seg, first, n in plan])
    keep = [c for c in range(len(plan)) if len(feats[c])]      # `if let Ok(embedding)`: a chunk without frames is dropped
    if not keep:
        return []
    emb = np.stack([np.asarray(emb_fn(feats[c]), np.float32).reshape(-1) for c in keep])
    labels = diarizer.cluster([emb], max(int(max_speakers), 1))[0][0]
    return speaker_segments([plan[c][0] for c in keep], [plan[c][1] for c in keep], labels, merge_gap)


def nme_sc(embeddings, max_speakers: int, device: int = 0) -> np.ndarray:
    """`nme_sc(&embeddings, max_speakers)` (diarization.rs:541): raw labels of one recording's [n, dim] embeddings."""
    d = Diarizer(device)
    try:
        return d.cluster([embeddings], max_speakers)[0][0]
    finally:
        d.close()


def chunk_plan(segments, sample_rate: int = 16000):
    """The ~4 s split of run_diarization (:311-338).  segments: (start, end, n_samples) triples ->
    list of (start, end, segment index, first sample, n samples)."""
    L = N.lib()
    s, e = _f64([x[0] for x in segments]), _f64([x[1] for x in segments])
    ns = np.ascontiguousarray([x[2] for x in segments], dtype=np.int64)
    args = (_p(s, C.c_double), _p(e, C.c_double), _p(ns, C.c_long), len(segments), int(sample_rate))
    cnt = L.crispy_diar_chunk_plan(*args, None, None, None, None, None, 0)
    if cnt < 0:
        N.check(int(cnt), L)
    os_, oe = np.zeros(cnt), np.zeros(cnt)
    og, of, ol = (np.zeros(cnt, np.int64) for _ in range(3))
    if cnt:
        L.crispy_diar_chunk_plan(*args, _p(os_, C.c_double), _p(oe, C.c_double), _p(og, C.c_long), _p(of, C.c_long), _p(ol, C.c_long), cnt)
    return [(float(os_[i]), float(oe[i]), int(og[i]), int(of[i]), int(ol[i])) for i in range(cnt)]


def speaker_segments(starts, ends, labels, merge_gap: float):
    """run_diarization's tail (:373-400): chunk times and raw labels -> merged [(start, end, speaker number >= 1)]."""
    L = N.lib()
    s, e, lb = _f64(starts), _f64(ends), np.ascontiguousarray(labels, dtype=np.int32)
    n = len(s)
    os_, oe, ow = np.zeros(n), np.zeros(n), np.zeros(n, np.int32)
    cnt = L.crispy_diar_speaker_segments(_p(s, C.c_double), _p(e, C.c_double), _p(lb, C.c_int), n, float(merge_gap),
                                         _p(os_, C.c_double), _p(oe, C.c_double), _p(ow, C.c_int), n)
    if cnt < 0:
        N.check(int(cnt), L)
    return [(float(os_[i]), float(oe[i]), int(ow[i])) for i in range(cnt)]


def _segs(segments):
    s, e = _f64([x[0] for x in segments]), _f64([x[1] for x in segments])
    w = np.ascontiguousarray([x[2] for x in segments], dtype=np.int32)
    return s, e, w, (_p(s, C.c_double), _p(e, C.c_double), _p(w, C.c_int), len(segments))


def speaker_name(s: int) -> str:
    return "Speaker ?" if s == 0 else f"Speaker {s}"


def find_speaker(time: float, segments) -> int:
    """find_speaker_at_time (:703-724); 0 stands for "Speaker ?"."""
    *_keep, args = _segs(segments)
    return int(N.lib().crispy_diar_find_speaker(float(time), *args))


def _text(call):
    L = N.lib()
    need = C.c_size_t(0)
    N.check(call(None, 0, C.byref(need)), L)
    buf = C.create_string_buffer(need.value)
    N.check(call(buf, need.value, C.byref(need)), L)
    return buf.value.decode("utf-8")


def format_diarized_text(words, segments) -> str:
    """format_diarized_text (:657-700).  words: (t0, t1, text) triples; segments: (start, end, speaker number)."""
    t0, t1 = _f64([w[0] for w in words]), _f64([w[1] for w in words])
    texts = (C.c_char_p * max(len(words), 1))(*[w[2].encode("utf-8") for w in words])
    *_keep, sa = _segs(segments)
    L = N.lib()
    return _text(lambda out, cap, need: L.crispy_diar_format_text(_p(t0, C.c_double), _p(t1, C.c_double), texts, len(words), *sa,
                                                                  out, cap, need))


def format_result(result_ptr, chunk_offset: float, segments) -> str:
    """The same over the words of a `crispy_asr_result *` (a transcribe call with dtw_token_timestamps)."""
    *_keep, sa = _segs(segments)
    L = N.lib()
    return _text(lambda out, cap, need: L.crispy_diar_format_result(result_ptr, float(chunk_offset), *sa, out, cap, need))
