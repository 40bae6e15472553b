"""Parakeet on the GPU (include/crispy_hip.h): the log-mel front end (crispy_pk_features*), 16 kHz mono f32 samples in, feature rows out;
the FastConformer encoder (crispy_pk_*), feature rows in, encoder frames out; the greedy TDT decoder (crispy_pk_tdt_*), frames in,
tokens with frame times and words out; and `Parakeet`, which owns both handles and goes from samples to words in one call
(crispy_pk_transcribe)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N

CONFIG_FIELDS = tuple(k for k, _t in N.PkConfig._fields_)


def _p(a, ty):
    return a.ctypes.data_as(C.POINTER(ty)) if a.size else None


def pk_frames(rows: int) -> int:
    """T' for `rows` feature rows (0 for rows < 1); no device"""
    return int(N.lib().crispy_pk_frames(int(rows)))


def pk_feature_rows(samples: int) -> int:
    """feature rows for `samples` samples at 16 kHz (samples // 160); no device"""
    return int(N.lib().crispy_pk_feature_rows(int(samples)))


def pk_mel_filters(mel_bins: int, lib=None) -> np.ndarray:
    """the built-in Slaney filters [mel_bins, 257] (crispy_pk_mel_filters); no device"""
    L = lib or N.lib()
    fb = np.zeros((max(int(mel_bins), 0), N.PK_MEL_SPEC), np.float32)
    N.check(L.crispy_pk_mel_filters(int(mel_bins), fb.ctypes.data if fb.size else None), L)
    return fb


def _sample_offsets(lengths):
    off = np.zeros(len(lengths) + 1, np.int64)
    off[1:] = np.cumsum(lengths)
    return off


def make_config(config) -> N.PkConfig:
    """a crispy_pk_config from a mapping or an object with the fields hidden, layers, heads, ffn, conv_kernel, mel_bins,
    sub_channels, attention_bias, convolution_bias, scale_input"""
    if isinstance(config, N.PkConfig):
        return config
    get = config.__getitem__ if hasattr(config, "__getitem__") else lambda k: getattr(config, k)
    return N.PkConfig(**{k: int(get(k)) for k in CONFIG_FIELDS})


def pk_tensor_spec(config, lib=None):
    """[(state-dict key, element count)] crispy_pk_load expects for `config`, in state-dict order; no device"""
    L = lib or N.lib()
    cfg = make_config(config)
    name, count = C.c_char_p(), C.c_long()
    n = L.crispy_pk_tensor_spec(C.byref(cfg), 0, C.byref(name), C.byref(count))
    N.check(0 if n > 0 else n, L)
    out = []
    for i in range(n):
        N.check(0 if L.crispy_pk_tensor_spec(C.byref(cfg), i, C.byref(name), C.byref(count)) == n else -1, L)
        out.append((name.value.decode("utf-8"), int(count.value)))
    return out


def state_dict_items(state_dict):
    """(key, f32 array) of an encoder's tensors from a torch or numpy state dict as it is: a leading `encoder.` is stripped,
    `num_batches_tracked` entries and the `encoder_projector.*` / `decoder.*` / `joint.*` keys of a ParakeetForTDT dict are dropped"""
    items = []
    for k, v in state_dict.items():
        k = str(k)
        if k.endswith("num_batches_tracked") or k.startswith(("encoder_projector.", "decoder.", "joint.")):
            continue
        if k.startswith("encoder."):
            k = k[len("encoder."):]
        if hasattr(v, "detach"):
            v = v.detach().cpu().float().numpy()
        items.append((k, np.ascontiguousarray(np.asarray(v, dtype=np.float32)).reshape(-1)))
    return items


class ParakeetEncoder:
    """A crispy_pk handle: its own stream, the loaded encoder and a workspace that grows on demand."""

    def __init__(self, device: int = 0, lib=None):
        self._L = lib or N.lib()
        self._h = C.c_void_p()
        N.check(self._L.crispy_pk_create(int(device), C.byref(self._h)), self._L)

    def close(self):
        if self._h:
            self._L.crispy_pk_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def load(self, config, state_dict):
        """The encoder's weights by their state-dict keys; a second load replaces the first."""
        cfg = make_config(config)
        items = state_dict_items(state_dict)
        n = len(items)
        names = (C.c_char_p * max(n, 1))(*[k.encode("utf-8") for k, _a in items])
        data = (C.c_void_p * max(n, 1))(*[a.ctypes.data for _k, a in items])
        count = np.ascontiguousarray([a.size for _k, a in items], dtype=np.int64)
        N.check(self._L.crispy_pk_load(self._h, C.byref(cfg), names, data, _p(count, C.c_long), n), self._L)

    @property
    def loaded(self) -> bool:
        return bool(self._L.crispy_pk_loaded(self._h))

    @property
    def config(self) -> dict:
        cfg = N.PkConfig()
        N.check(self._L.crispy_pk_config_of(self._h, C.byref(cfg)), self._L)
        return {k: int(getattr(cfg, k)) for k in CONFIG_FIELDS}

    def set_precision(self, mode: int):
        """0: f32 operands (the default).  1: f16 operands with f32 sums in every GEMM of the encoder (crispy_pk_set_precision); before
        or after a load, and kept across loads."""
        N.check(self._L.crispy_pk_set_precision(self._h, int(mode)), self._L)

    @property
    def precision(self) -> int:
        return int(self._L.crispy_pk_precision(self._h))

    def stage_gemm_device(self, mode: int, epilogue: int, a, w, bias=None, alpha: float = 1.0, res=None):
        """One GEMM of the encoder as a stage (crispy_pk_stage_gemm_device; needs no load): CUDA f32 tensors a [M, K], w in the
        state-dict layout [cols, K] (cols = 2 N with N.PK_GEMM_GLU), bias [cols] or None, res [M, N] for N.PK_GEMM_RESIDUAL ->
        a CUDA tensor [M, N]."""
        import torch
        a, w = a.contiguous(), w.contiguous()
        if a.dtype != torch.float32 or w.dtype != torch.float32 or a.dim() != 2 or w.dim() != 2:
            raise ValueError("a and w must be f32 matrices")
        M, K = int(a.shape[0]), int(a.shape[1])
        cols = int(w.shape[0])
        n = cols // 2 if int(epilogue) == N.PK_GEMM_GLU else cols
        bias = bias.contiguous() if bias is not None else None
        res = res.contiguous() if res is not None else None
        out = torch.empty((M, n), dtype=torch.float32, device=a.device)
        torch.cuda.current_stream(a.device).synchronize()      # the handle's stream does not wait for torch's
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
        N.check(self._L.crispy_pk_stage_gemm_device(self._h, int(mode), int(epilogue), ptr(a), M, K, ptr(w), ptr(bias), n, float(alpha), ptr(res),
                                                    ptr(out)), self._L)
        return out

    def stage_gemm(self, mode: int, epilogue: int, a, w, bias=None, alpha: float = 1.0, res=None, device="cuda"):
        """The same on numpy arrays -> a numpy array (the copies go through torch; the library has the device form only)."""
        import torch
        up = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(device)
        return self.stage_gemm_device(mode, epilogue, up(a), up(w), up(bias), alpha, up(res)).cpu().numpy()

    def set_attention_precision(self, mode: int):
        """0: f32 operands in the attention's three products (the default).  1: q + u, q + v, k, r, v and the soft-max weights rounded
        once to f16, f32 sums, the soft-max in key tiles of N.PK_ATTN_KEY_TILE (crispy_pk_set_attention_precision).  Independent of
        set_precision; before or after a load, and kept across loads."""
        N.check(self._L.crispy_pk_set_attention_precision(self._h, int(mode)), self._L)

    @property
    def attention_precision(self) -> int:
        return int(self._L.crispy_pk_attention_precision(self._h))

    def stage_attention_device(self, mode: int, qkv, r, bias_u, bias_v, lengths, heads: int, tmax: int):
        """One attention pass as a stage (crispy_pk_stage_attention_device; needs no load): CUDA f32 tensors qkv [sum n, 3 * heads * 128]
        (q | k | v side by side), r [2 tmax - 1, heads * 128] (row p for the distance p - (tmax - 1)), bias_u and bias_v
        [heads * 128]; `lengths` the clips' frame counts -> a CUDA tensor [sum n, heads * 128]."""
        import torch
        def prep(t):      # contiguous f32 on a 16-byte boundary
            if t.dtype != torch.float32:
                raise ValueError("the operands must be f32")
            t = t.contiguous()
            return t.clone() if t.data_ptr() % 16 else t
        qkv, r, bias_u, bias_v = prep(qkv), prep(r), prep(bias_u), prep(bias_v)
        off = _sample_offsets([int(n) for n in lengths])
        n = len(lengths)
        out = torch.empty((max(int(off[-1]), 1), max(int(heads), 1) * N.PK_HEAD_DIM), dtype=torch.float32, device=qkv.device)      # never empty: the library refuses heads itself
        torch.cuda.current_stream(qkv.device).synchronize()      # the handle's stream does not wait for torch's
        ptr = lambda t: t.data_ptr() if t.numel() else None
        N.check(self._L.crispy_pk_stage_attention_device(self._h, int(mode), ptr(qkv), ptr(r), ptr(bias_u), ptr(bias_v), _p(off, C.c_long) if n else None,
                                                         n, int(heads), int(tmax), ptr(out)), self._L)
        return out[:int(off[-1])] if int(heads) >= 1 else out[:0]

    def stage_attention(self, mode: int, qkv, r, bias_u, bias_v, lengths, heads: int, tmax: int, device="cuda"):
        """The same on numpy arrays -> a numpy array (the copies go through torch; the library has the device form only)."""
        import torch
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(device)
        return self.stage_attention_device(mode, up(qkv), up(r), up(bias_u), up(bias_v), lengths, heads, tmax).cpu().numpy()

    def _shape(self):
        if not self.loaded:      # the library refuses the call with its own message; the buffers need no width for that
            return 1, 1
        c = self.config
        return c["hidden"], c["mel_bins"]

    def set_mel_filters(self, fb=None):
        """Replaces the front end's built-in Slaney filters with `fb` [mel_bins, 257] (a checkpoint's own featurizer.fb); None restores
        them."""
        if fb is None:
            N.check(self._L.crispy_pk_set_mel_filters(self._h, 0, None), self._L)
            return
        if hasattr(fb, "detach"):
            fb = fb.detach().cpu().float().numpy()
        fb = np.ascontiguousarray(fb, dtype=np.float32)
        if fb.ndim != 2 or fb.shape[1] != N.PK_MEL_SPEC:
            raise ValueError("filters must be [mel_bins, 257]")
        N.check(self._L.crispy_pk_set_mel_filters(self._h, int(fb.shape[0]), fb.ctypes.data), self._L)

    def _mel_bins(self, mel_bins):
        if mel_bins is not None:
            return int(mel_bins)
        if not self.loaded:
            raise ValueError("mel_bins is needed before a load")
        return self.config["mel_bins"]

    def features_device(self, pcm_list, mel_bins=None, taps: bool = False, stream=None):
        """Clips as CUDA f32 tensors of 16 kHz mono samples in one ragged call -> a list of CUDA tensors [rows, mel_bins], what
        encode_device takes; with `taps` a tuple (rows, rows before normalisation, (mean, std) [2, mel_bins] per clip).  `mel_bins`
        defaults to the loaded encoder's."""
        import torch
        M = self._mel_bins(mel_bins)
        clips = [p.reshape(-1) for p in pcm_list]
        dev = clips[0].device if clips else torch.device("cuda")
        x = torch.cat(clips, 0).contiguous() if clips else torch.zeros((0,), dtype=torch.float32, device=dev)
        if x.dtype != torch.float32:
            raise ValueError("samples must be f32")
        n = len(clips)
        off = _sample_offsets([int(c.shape[0]) for c in clips])
        q = _sample_offsets([pk_feature_rows(int(c.shape[0])) for c in clips])
        width = max(M, 0)
        out = torch.empty((int(q[-1]), width), dtype=torch.float32, device=dev)
        raw = torch.empty((int(q[-1]), width), dtype=torch.float32, device=dev) if taps else None
        stats = torch.empty((n, 2, width), dtype=torch.float32, device=dev) if taps else None
        if stream is None:      # the handle's stream does not wait for torch's
            torch.cuda.current_stream(dev).synchronize()
        ptr = lambda a: a.data_ptr() if a is not None and a.numel() else None
        N.check(self._L.crispy_pk_features_device(self._h, M, ptr(x), _p(off, C.c_long) if n else None, n, ptr(out), ptr(raw), ptr(stats), stream),
                self._L)
        cut = lambda a: [a[q[c]:q[c + 1]] for c in range(n)]
        return (cut(out), cut(raw), [stats[c] for c in range(n)]) if taps else cut(out)

    def features(self, pcm_list, mel_bins=None, taps: bool = False):
        """The same on numpy arrays through the library's host form (crispy_pk_features) -> numpy arrays."""
        M = self._mel_bins(mel_bins)
        clips = [np.ascontiguousarray(p, dtype=np.float32).reshape(-1) for p in pcm_list]
        x = np.ascontiguousarray(np.concatenate(clips)) if clips else np.zeros(0, np.float32)
        n = len(clips)
        off = _sample_offsets([c.shape[0] for c in clips])
        q = _sample_offsets([pk_feature_rows(int(c.shape[0])) for c in clips])
        width = max(M, 0)
        out = np.zeros((int(q[-1]), width), np.float32)
        raw = np.zeros((int(q[-1]), width), np.float32) if taps else None
        stats = np.zeros((n, 2, width), np.float32) if taps else None
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None
        N.check(self._L.crispy_pk_features(self._h, M, ptr(x), _p(off, C.c_long) if n else None, n, ptr(out), ptr(raw), ptr(stats)), self._L)
        cut = lambda a: [a[q[c]:q[c + 1]] for c in range(n)]
        return (cut(out), cut(raw), [stats[c] for c in range(n)]) if taps else cut(out)

    def encode_device(self, feats_list, taps: bool = False, tap_layer: int = 0, stream=None):
        """Clips as CUDA f32 tensors [rows, M] in one ragged call -> a list of CUDA tensors [T', H]; with `taps` a tuple (frames,
        subsampling outputs, outputs of block `tap_layer`, position table [2 Tmax - 1, H])."""
        import torch
        H, M = self._shape()
        rows = [f.reshape(-1, M) for f in feats_list]
        dev = rows[0].device if rows else torch.device("cuda")
        x = torch.cat(rows, 0).contiguous() if rows else torch.zeros((0, M), dtype=torch.float32, device=dev)
        if x.dtype != torch.float32:
            raise ValueError("features must be f32 [rows, mel_bins]")
        n = len(rows)
        off = np.zeros(n + 1, np.int64)
        off[1:] = np.cumsum([int(r.shape[0]) for r in rows])
        t = [pk_frames(int(r.shape[0])) for r in rows]
        q = np.concatenate([[0], np.cumsum(t)]).astype(np.int64)
        total, tmax = int(q[-1]), max(t, default=0)
        new = lambda r: torch.empty((r, H), dtype=torch.float32, device=dev)
        out = new(total)
        sub, tap, pos = (new(total), new(total), new(max(2 * tmax - 1, 0))) if taps else (None, None, None)
        if stream is None:      # the handle's stream does not wait for torch's
            torch.cuda.current_stream(dev).synchronize()
        ptr = lambda a: a.data_ptr() if a is not None and a.numel() else None
        N.check(self._L.crispy_pk_encode_device(self._h, ptr(x), _p(off, C.c_long) if n else None, n, ptr(out), ptr(sub), int(tap_layer), ptr(tap),
                                                ptr(pos), stream), self._L)
        cut = lambda a: [a[q[c]:q[c + 1]] for c in range(n)]
        return (cut(out), cut(sub), cut(tap), pos) if taps else cut(out)

    def encode(self, feats_list, taps: bool = False, tap_layer: int = 0):
        """The same on numpy arrays through the library's host form (crispy_pk_encode) -> numpy arrays."""
        H, M = self._shape()
        rows = [np.ascontiguousarray(f, dtype=np.float32).reshape(-1, M) for f in feats_list]
        x = np.ascontiguousarray(np.concatenate(rows, 0)) if rows else np.zeros((0, M), np.float32)
        n = len(rows)
        off = np.zeros(n + 1, np.int64)
        off[1:] = np.cumsum([r.shape[0] for r in rows])
        t = [pk_frames(int(r.shape[0])) for r in rows]
        q = np.concatenate([[0], np.cumsum(t)]).astype(np.int64)
        total, tmax = int(q[-1]), max(t, default=0)
        new = lambda r: np.zeros((r, H), np.float32)
        out = new(total)
        sub, tap, pos = (new(total), new(total), new(max(2 * tmax - 1, 0))) if taps else (None, None, None)
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None
        N.check(self._L.crispy_pk_encode(self._h, ptr(x), _p(off, C.c_long) if n else None, n, ptr(out), ptr(sub), int(tap_layer), ptr(tap),
                                         ptr(pos)), self._L)
        cut = lambda a: [a[q[c]:q[c + 1]] for c in range(n)]
        return (cut(out), cut(sub), cut(tap), pos) if taps else cut(out)


# ---- the TDT decoder ---------------------------------------------------------------------------------------------------------
TDT_CONFIG_FIELDS = tuple(k for k, _t in N.PkTdtConfig._fields_)
TDT_PREFIXES = ("encoder_projector.", "decoder.", "joint.")


def make_tdt_config(config) -> N.PkTdtConfig:
    """a crispy_pk_tdt_config from a mapping or an object with the fields hidden, decoder_hidden, decoder_layers, vocab, blank,
    durations (a sequence; n_durations is its length unless given) and max_symbols_per_step"""
    if isinstance(config, N.PkTdtConfig):
        return config
    get = config.__getitem__ if hasattr(config, "__getitem__") else lambda k: getattr(config, k)
    has = (lambda k: k in config) if hasattr(config, "__contains__") else (lambda k: hasattr(config, k))
    dur = [int(d) for d in get("durations")]
    n = int(get("n_durations")) if has("n_durations") else len(dur)
    if len(dur) > 8:
        raise ValueError("at most 8 durations")
    cfg = N.PkTdtConfig(**{k: int(get(k)) for k in TDT_CONFIG_FIELDS if k not in ("durations", "n_durations")})
    cfg.n_durations = n
    cfg.durations = (C.c_int * 8)(*(dur + [0] * (8 - len(dur))))
    return cfg


def _tdt_config_dict(cfg: N.PkTdtConfig) -> dict:
    out = {k: int(getattr(cfg, k)) for k in TDT_CONFIG_FIELDS if k != "durations"}
    out["durations"] = [int(d) for d in cfg.durations]
    return out


def pk_tdt_max_steps(config, frames: int, lib=None) -> int:
    """the step budget of one clip of `frames` frames; no device"""
    L = lib or N.lib()
    cfg = make_tdt_config(config)
    n = int(L.crispy_pk_tdt_max_steps(C.byref(cfg), int(frames)))
    N.check(0 if n >= 0 else n, L)
    return n


def pk_tdt_tensor_spec(config, lib=None):
    """[(state-dict key, element count)] crispy_pk_tdt_load expects for `config`, in state-dict order; no device"""
    L = lib or N.lib()
    cfg = make_tdt_config(config)
    name, count = C.c_char_p(), C.c_long()
    n = L.crispy_pk_tdt_tensor_spec(C.byref(cfg), 0, C.byref(name), C.byref(count))
    N.check(0 if n > 0 else n, L)
    out = []
    for i in range(n):
        N.check(0 if L.crispy_pk_tdt_tensor_spec(C.byref(cfg), i, C.byref(name), C.byref(count)) == n else -1, L)
        out.append((name.value.decode("utf-8"), int(count.value)))
    return out


def tdt_state_dict_items(state_dict):
    """(key, f32 array) of the decoder's tensors from a torch or numpy ParakeetForTDT state dict as it is: the `encoder_projector.*`,
    `decoder.*` and `joint.*` keys; the encoder's are dropped"""
    items = []
    for k, v in state_dict.items():
        k = str(k)
        if not k.startswith(TDT_PREFIXES):
            continue
        if hasattr(v, "detach"):
            v = v.detach().cpu().float().numpy()
        items.append((k, np.ascontiguousarray(np.asarray(v, dtype=np.float32)).reshape(-1)))
    return items


def pk_tdt_words(steps, pieces, frames: int, blank: int, seconds_per_frame: float = 0.08, lib=None):
    """One clip's steps [n][3] and the vocabulary's pieces -> [(start_s, end_s, text)] (crispy_pk_tdt_words); no device"""
    L = lib or N.lib()
    steps = np.ascontiguousarray(steps, dtype=np.int32).reshape(-1, 3)
    raw = (C.c_char_p * max(len(pieces), 1))(*[p.encode("utf-8") if isinstance(p, str) else bytes(p) for p in pieces])
    need = C.c_long()
    args = (steps.ctypes.data if len(steps) else None, len(steps), int(frames), int(blank), raw, len(pieces), float(seconds_per_frame))
    n = int(L.crispy_pk_tdt_words(*args, None, None, None, 0, None, 0, C.byref(need)))
    N.check(0 if n >= 0 else n, L)
    if n == 0:
        return []
    start, end, off = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.int64)
    text = C.create_string_buffer(int(need.value))
    got = int(L.crispy_pk_tdt_words(*args, start.ctypes.data, end.ctypes.data, off.ctypes.data, n, text, int(need.value), C.byref(need)))
    N.check(0 if got == n else min(got, -1), L)
    raw_text = text.raw
    return [(start[i], end[i], raw_text[off[i]:raw_text.index(b"\0", off[i])].decode("utf-8")) for i in range(n)]


class ParakeetTDT:
    """A crispy_pk_tdt handle: its own stream, the loaded decoder and a workspace that grows on demand."""

    def __init__(self, device: int = 0, lib=None):
        self._L = lib or N.lib()
        self._h = C.c_void_p()
        N.check(self._L.crispy_pk_tdt_create(int(device), C.byref(self._h)), self._L)

    def close(self):
        if self._h:
            self._L.crispy_pk_tdt_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def load(self, config, state_dict):
        """The decoder's weights by their state-dict keys (a whole ParakeetForTDT dict is fine); a second load replaces the first."""
        cfg = make_tdt_config(config)
        items = tdt_state_dict_items(state_dict)
        n = len(items)
        names = (C.c_char_p * max(n, 1))(*[k.encode("utf-8") for k, _a in items])
        data = (C.c_void_p * max(n, 1))(*[a.ctypes.data for _k, a in items])
        count = np.ascontiguousarray([a.size for _k, a in items], dtype=np.int64)
        N.check(self._L.crispy_pk_tdt_load(self._h, C.byref(cfg), names, data, _p(count, C.c_long), n), self._L)

    @property
    def loaded(self) -> bool:
        return bool(self._L.crispy_pk_tdt_loaded(self._h))

    @property
    def config(self) -> dict:
        cfg = N.PkTdtConfig()
        N.check(self._L.crispy_pk_tdt_config_of(self._h, C.byref(cfg)), self._L)
        return _tdt_config_dict(cfg)

    def _shape(self):
        """(H, D, V + n_d, [budget(T') for a clip]) of the loaded decoder; before a load the library refuses the call itself"""
        if not self.loaded:
            return 1, 1, 1, lambda t: 0
        cfg = N.PkTdtConfig()
        N.check(self._L.crispy_pk_tdt_config_of(self._h, C.byref(cfg)), self._L)
        m = int(cfg.max_symbols_per_step)
        return int(cfg.hidden), int(cfg.decoder_hidden), int(cfg.vocab) + int(cfg.n_durations), lambda t: max(0, m * t - 1) if 0 < t <= 5000 else 0

    @staticmethod
    def _offsets(lengths, budget):
        off = np.zeros(len(lengths) + 1, np.int64)
        off[1:] = np.cumsum(lengths)
        q = np.zeros(len(lengths) + 1, np.int64)
        q[1:] = np.cumsum([budget(int(t)) for t in lengths])
        return off, q

    def decode_device(self, frames_list, taps: bool = False, stream=None):
        """Clips as CUDA f32 tensors [T', H] in one ragged call -> a list of CUDA int32 tensors [n_steps, 3] (token, frame, duration);
        with `taps` a tuple (steps, projected frames [T', D] per clip, logits [n_steps, V + n_d] per clip)."""
        import torch
        H, D, W, budget = self._shape()
        rows = [f.reshape(-1, H) for f in frames_list]
        dev = rows[0].device if rows else torch.device("cuda")
        x = torch.cat(rows, 0).contiguous() if rows else torch.zeros((0, H), dtype=torch.float32, device=dev)
        if x.dtype != torch.float32:
            raise ValueError("frames must be f32 [T', hidden]")
        n = len(rows)
        off, q = self._offsets([int(r.shape[0]) for r in rows], budget)
        steps = torch.zeros((int(q[-1]), 3), dtype=torch.int32, device=dev)
        n_steps = torch.zeros((max(n, 1),), dtype=torch.int32, device=dev)
        proj = torch.zeros((int(off[-1]), D), dtype=torch.float32, device=dev) if taps else None
        logits = torch.zeros((int(q[-1]), W), dtype=torch.float32, device=dev) if taps else None
        if stream is None:      # the handle's stream does not wait for torch's
            torch.cuda.current_stream(dev).synchronize()
        ptr = lambda a: a.data_ptr() if a is not None and a.numel() else None
        N.check(self._L.crispy_pk_tdt_decode_device(self._h, ptr(x), _p(off, C.c_long) if n else None, n, ptr(steps), n_steps.data_ptr(), ptr(proj),
                                                    ptr(logits), stream), self._L)
        cnt = n_steps.cpu().numpy()
        cut = lambda a, at, length: [a[at[c]:at[c] + length[c]] for c in range(n)]
        out = cut(steps, q, cnt)
        return (out, cut(proj, off, np.diff(off)), cut(logits, q, cnt)) if taps else out

    def decode(self, frames_list, taps: bool = False):
        """The same on numpy arrays through the library's host form (crispy_pk_tdt_decode) -> numpy arrays."""
        H, D, W, budget = self._shape()
        rows = [np.ascontiguousarray(f, dtype=np.float32).reshape(-1, H) for f in frames_list]
        x = np.ascontiguousarray(np.concatenate(rows, 0)) if rows else np.zeros((0, H), np.float32)
        n = len(rows)
        off, q = self._offsets([r.shape[0] for r in rows], budget)
        steps = np.zeros((int(q[-1]), 3), np.int32)
        n_steps = np.zeros(max(n, 1), np.int32)
        proj = np.zeros((int(off[-1]), D), np.float32) if taps else None
        logits = np.zeros((int(q[-1]), W), np.float32) if taps else None
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None
        N.check(self._L.crispy_pk_tdt_decode(self._h, ptr(x), _p(off, C.c_long) if n else None, n, ptr(steps), n_steps.ctypes.data, ptr(proj),
                                             ptr(logits)), self._L)
        cut = lambda a, at, length: [a[at[c]:at[c] + length[c]] for c in range(n)]
        out = cut(steps, q, n_steps)
        return (out, cut(proj, off, np.diff(off)), cut(logits, q, n_steps)) if taps else out

    @staticmethod
    def words(steps, pieces, frames: int, blank: int, seconds_per_frame: float = 0.08):
        """[(start_s, end_s, text)] of one clip's steps (pk_tdt_words)"""
        return pk_tdt_words(steps, pieces, frames, blank, seconds_per_frame)


# ---- samples to words ---------------------------------------------------------------------------------------------------------
class Parakeet:
    """The whole arm: a ParakeetEncoder (with its log-mel front end) and a ParakeetTDT on one device, and crispy_pk_transcribe over both."""

    def __init__(self, device: int = 0, lib=None):
        self._L = lib or N.lib()
        self.encoder = ParakeetEncoder(device, self._L)
        self.decoder = ParakeetTDT(device, self._L)

    def close(self):
        self.encoder.close()
        self.decoder.close()

    def set_precision(self, mode: int):
        """The encoder's precision mode (ParakeetEncoder.set_precision); the front end and the decoder stay f32."""
        self.encoder.set_precision(mode)

    def set_attention_precision(self, mode: int):
        """The encoder's attention mode (ParakeetEncoder.set_attention_precision), independent of set_precision."""
        self.encoder.set_attention_precision(mode)

    def load(self, config, tdt_config, state_dict):
        """One ParakeetForTDT state dict: the `encoder.*` keys go to the encoder, the rest to the decoder."""
        self.encoder.load(config, state_dict)
        self.decoder.load(tdt_config, state_dict)

    def _layout(self, lengths):
        """sample offsets, the frames of each clip and the first row of each clip in the step log"""
        _h, _d, _w, budget = self.decoder._shape()
        off = _sample_offsets(lengths)
        frames = [pk_frames(pk_feature_rows(int(n))) for n in lengths]
        q = _sample_offsets([budget(t) for t in frames])
        return off, frames, q

    def _result(self, steps, frames, pieces):
        out = []
        blank = self.decoder.config["blank"] if pieces is not None else 0
        for s, t in zip(steps, frames):
            r = {"steps": s}
            if pieces is not None:
                r["words"] = pk_tdt_words(s, pieces, t, blank, lib=self._L)
                r["text"] = " ".join(w for _a, _b, w in r["words"]).strip()
            out.append(r)
        return out

    def transcribe(self, pcm_list, pieces=None):
        """Clips of 16 kHz mono f32 samples (numpy) in one ragged call (crispy_pk_transcribe) -> per clip a dict with `steps`
        [n_steps, 3] (token, frame, duration); with the vocabulary's `pieces` also `words` [(start_s, end_s, text)] and `text`, the
        words joined by one space."""
        clips = [np.ascontiguousarray(p, dtype=np.float32).reshape(-1) for p in pcm_list]
        x = np.ascontiguousarray(np.concatenate(clips)) if clips else np.zeros(0, np.float32)
        n = len(clips)
        off, frames, q = self._layout([c.shape[0] for c in clips])
        steps = np.zeros((int(q[-1]), 3), np.int32)
        n_steps = np.zeros(max(n, 1), np.int32)
        ptr = lambda a: a.ctypes.data if a.size else None
        N.check(self._L.crispy_pk_transcribe(self.encoder._h, self.decoder._h, ptr(x), _p(off, C.c_long) if n else None, n, ptr(steps),
                                             n_steps.ctypes.data), self._L)
        return self._result([steps[q[c]:q[c] + n_steps[c]] for c in range(n)], frames, pieces)

    def transcribe_device(self, pcm_list, pieces=None, stream=None):
        """The same on CUDA f32 tensors (crispy_pk_transcribe_device); `steps` are CUDA int32 tensors."""
        import torch
        clips = [p.reshape(-1) for p in pcm_list]
        dev = clips[0].device if clips else torch.device("cuda")
        x = torch.cat(clips, 0).contiguous() if clips else torch.zeros((0,), dtype=torch.float32, device=dev)
        if x.dtype != torch.float32:
            raise ValueError("samples must be f32")
        n = len(clips)
        off, frames, q = self._layout([int(c.shape[0]) for c in clips])
        steps = torch.zeros((int(q[-1]), 3), dtype=torch.int32, device=dev)
        n_steps = torch.zeros((max(n, 1),), dtype=torch.int32, device=dev)
        if stream is None:      # the handles' streams do not wait for torch's
            torch.cuda.current_stream(dev).synchronize()
        ptr = lambda a: a.data_ptr() if a.numel() else None
        N.check(self._L.crispy_pk_transcribe_device(self.encoder._h, self.decoder._h, ptr(x), _p(off, C.c_long) if n else None, n, ptr(steps),
                                                    n_steps.data_ptr(), stream), self._L)
        cnt = n_steps.cpu().numpy()
        cut = [steps[q[c]:q[c] + cnt[c]] for c in range(n)]
        if pieces is None:
            return self._result(cut, frames, None)
        return self._result([s.cpu().numpy() for s in cut], frames, pieces)
