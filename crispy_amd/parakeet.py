"""The Parakeet FastConformer encoder on the GPU (crispy_pk_*, include/crispy_hip.h): log-mel feature rows in, encoder frames out.
The log-mel front end and the TDT decoder are not part of it."""
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
    `num_batches_tracked` entries and the `decoder.*` / `joint.*` keys of a ParakeetForTDT dict are dropped"""
    items = []
    for k, v in state_dict.items():
        k = str(k)
        if k.endswith("num_batches_tracked") or k.startswith(("decoder.", "joint.")):
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

    def _shape(self):
        if not self.loaded:      # the library refuses the call with its own message; the buffers need no width for that
            return 1, 1
        c = self.config
        return c["hidden"], c["mel_bins"]

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
