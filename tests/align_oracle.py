"""Oracle of the word-level alignment (crispy_asr_opts::dtw_token_timestamps): openai-whisper's find_alignment /
add_word_timestamps recipe restated in numpy [UPSTREAM-RECALL: whisper/timing.py, whisper/tokenizer.py].

  alignment(...)        teacher-forced float64 decoder (oracle.whisper_oracle.DecoderCache, f16=True: precision mode 1's
                        operands) recording the cross-attention scores; softmax over the first n_frames // 2 keys of every
                        alignment head, standardised per frame over the token rows (population std), 7-wide median filter
                        with reflect padding, mean over the heads
  dtw(x)                openai's dtw_cpu + backtrace: f32 costs, ties to the left
  jump_indices(...)     the path's entry column of every row
  split_words(...)      split_tokens_on_unicode / split_tokens_on_spaces on the tokens' byte strings
  merge_punctuations    openai's, default sets; returns the words it keeps
"""
import string

import numpy as np

from oracle.whisper_oracle import DecoderCache


class RecordingDecoder(DecoderCache):
    """DecoderCache that keeps every cross-attention score row: qk[layer] = list of [n_head][Tn] arrays, one per step."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.qk = [[] for _ in range(self.hp.n_text_layer)]

    def _att(self, q, k, v):
        for i, xk in enumerate(self.xk):
            if k is xk:
                H = self.hp.n_text_head
                dh = q.shape[-1] // H
                rows = []
                for h in range(H):
                    sl = slice(h * dh, (h + 1) * dh)
                    qh = q[sl].astype(np.float16).astype(q.dtype) if self.attn16 else q[sl]
                    rows.append((k[:, sl] @ qh) / q.dtype.type(np.sqrt(dh)))
                self.qk[i].append(np.stack(rows))
                break
        return super()._att(q, k, v)


def default_heads(hp):
    return [(l, h) for l in range(hp.n_text_layer // 2, hp.n_text_layer) for h in range(hp.n_text_head)]


def median_filter(x, width=7):
    """openai's median_filter: reflect padding along the last axis, the middle of each window of `width`."""
    pad = width // 2
    xp = np.pad(x, [(0, 0)] * (x.ndim - 1) + [(pad, pad)], mode="reflect")
    win = np.lib.stride_tricks.sliding_window_view(xp, width, axis=-1)
    return np.sort(win, axis=-1)[..., pad]


def matrix_from_scores(qk, n_frames):
    """qk [n_heads][rows][Tn] raw scores -> (probs [n_heads][rows][F], matrix [rows][F]); float64."""
    F = n_frames // 2
    w = qk[:, :, :F]
    w = np.exp(w - w.max(-1, keepdims=True))
    probs = w / w.sum(-1, keepdims=True)
    mean = probs.mean(-2, keepdims=True)
    std = probs.std(-2, keepdims=True)
    z = (probs - mean) / std
    return probs, median_filter(z, 7).mean(0)


def alignment(weights, hp, enc_out, tokens, n_frames, heads=None, f16=False, attn16=False):
    heads = heads or default_heads(hp)
    dc = RecordingDecoder(weights, hp, enc_out, f16=f16, attn16=attn16)
    for t in tokens:
        dc.step(t)
    qk = np.stack([np.stack(dc.qk[l])[:, h, :] for l, h in heads])      # [n_heads][rows][Tn]
    return matrix_from_scores(qk, n_frames)


def dtw(x):
    """openai's dtw_cpu + backtrace on x [N][M]: returns (text_indices, time_indices)."""
    x = np.asarray(x, np.float32)
    N, M = x.shape
    cost = np.full((N + 1, M + 1), np.inf, np.float32)
    trace = -np.ones((N + 1, M + 1), np.int8)
    cost[0, 0] = 0
    for j in range(1, M + 1):
        for i in range(1, N + 1):
            c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
            if c0 < c1 and c0 < c2:
                c, t = c0, 0
            elif c1 < c0 and c1 < c2:
                c, t = c1, 1
            else:
                c, t = c2, 2
            cost[i, j] = np.float32(x[i - 1, j - 1] + c)
            trace[i, j] = t
    i, j = N, M
    trace[0, :] = 2
    trace[:, 0] = 1
    res = []
    while i > 0 or j > 0:
        res.append((i - 1, j - 1))
        if trace[i, j] == 0:
            i, j = i - 1, j - 1
        elif trace[i, j] == 1:
            i -= 1
        else:
            j -= 1
    res = np.array(res[::-1]).T
    return res[0], res[1]


def jump_indices(text_idx, time_idx):
    jumps = np.pad(np.diff(text_idx), (1, 0), constant_values=1).astype(bool)
    return time_idx[jumps]


def token_time(seek, idx):
    """The library's token / word time: float32(seek x 0.01 + index x 0.02), computed in float64."""
    return np.float32(seek * 0.01 + int(idx) * 0.02)


def split_words(pieces, unicode_only=False):
    """pieces: the text tokens' byte strings -> [(word bytes, first, n)] (split_tokens_on_unicode, then
    split_tokens_on_spaces unless unicode_only)."""
    full = b"".join(pieces).decode("utf-8", "replace")
    units, cur, off = [], [], 0
    for k in range(len(pieces)):
        cur.append(k)
        dec = b"".join(pieces[i] for i in cur).decode("utf-8", "replace")
        if "\ufffd" not in dec or full[off + dec.index("\ufffd")] == "\ufffd":
            units.append((dec, cur[0], len(cur)))
            off += len(dec)
            cur = []
    if cur:
        dec = b"".join(pieces[i] for i in cur).decode("utf-8", "replace")
        units.append((dec, cur[0], len(cur)))
    if unicode_only:
        return [[u, f, n] for u, f, n in units]
    words = []
    for u, f, n in units:
        if u.startswith(" ") or u.strip() in string.punctuation or not words:
            words.append([u, f, n])
        else:
            words[-1][0] += u
            words[-1][2] += n
    return words


def merge_punctuations(words, prepended="\"'\u201c\u00bf([{-", appended="\"'.\u3002,\uff0c!\uff01?\uff1f:\uff1a\u201d)]}\u3001"):
    """words: [[text, first, n, t0, t1]] -> the kept words after openai's merge (times stay with the word they belong to)."""
    w = [list(x) for x in words]
    i, j = len(w) - 2, len(w) - 1
    while i >= 0:
        prev, nxt = w[i], w[j]
        if prev[0].startswith(" ") and prev[0].strip() in prepended:
            nxt[0] = prev[0] + nxt[0]
            if prev[2]:
                nxt[1], nxt[2] = prev[1], nxt[2] + prev[2]
            prev[0], prev[2] = "", 0
        else:
            j = i
        i -= 1
    i, j = 0, 1
    while j < len(w):
        prev, nxt = w[i], w[j]
        if not prev[0].endswith(" ") and nxt[0] in appended:
            prev[0] = prev[0] + nxt[0]
            if nxt[2]:
                if not prev[2]:
                    prev[1] = nxt[1]
                prev[2] += nxt[2]
            nxt[0], nxt[2] = "", 0
        else:
            i = j
        j += 1
    return [x for x in w if x[0]]


def window_words(pieces, idx, seek, unicode_only=False):
    """The words of one aligned window as the library reports them: [(t0, t1, text, first, n)] with first / n counted in
    the window's text tokens."""
    ws = split_words(pieces, unicode_only)
    ws = [[t, f, n, token_time(seek, idx[f]), token_time(seek, idx[f + n])] for t, f, n in ws]
    return [(t0, t1, t, f, n) for t, f, n, t0, t1 in merge_punctuations(ws)]
