"""CPU tests of the recording leg's host side (crispy_rn_record_* / crispy_rn_level* / crispy_record_worker_plan,
include/crispy_hip.h): the entry points validate without a device, the binding knows them, the worker plan equals the
oracle's loop, the oracle's quantiser gives the vectors the reference itself holds, the kernels of rn_record.hip
(cross-compiled here) use no scratch and contract no multiply-add, and WavWriter writes the reference's WAV spec."""
import ctypes as C
import os
import re
import subprocess
import wave

import numpy as np
import pytest

from tests import record_oracle as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
HANDLE_NAMES = ("crispy_rn_record_configure", "crispy_rn_record_app_push_device", "crispy_rn_record_app_push",
                "crispy_rn_level_device", "crispy_rn_level", "crispy_rn_record_buffered", "crispy_rn_record_frames_ready",
                "crispy_rn_record_drain_device", "crispy_rn_record_drain")
NAMES = HANDLE_NAMES + ("crispy_record_worker_plan",)
FMA = r"\bv_(fma|fmac|mad|mac|pk_fma)_(f32|f16|legacy|mix)"


def _lib():
    from crispy_amd import _native as N
    return N.lib()


# ---- 1 -------------------------------------------------------------------------------------------------------------
def test_entry_points_validate_without_a_device():
    L = _lib()
    n, mic, app = C.c_long(7), C.c_long(7), C.c_long(7)
    buf = (C.c_float * 16)()
    p = C.addressof(buf)
    calls = {
        "crispy_rn_record_configure": lambda: L.crispy_rn_record_configure(None, 0),
        "crispy_rn_record_app_push_device": lambda: L.crispy_rn_record_app_push_device(None, p, 4, 2, 2, None),
        "crispy_rn_record_app_push": lambda: L.crispy_rn_record_app_push(None, p, 4, 2, 2),
        "crispy_rn_level_device": lambda: L.crispy_rn_level_device(None, p, 4, 4, p, None),
        "crispy_rn_level": lambda: L.crispy_rn_level(None, p, 4, 4, p),
        "crispy_rn_record_buffered": lambda: L.crispy_rn_record_buffered(None, C.byref(mic), C.byref(app)),
        "crispy_rn_record_frames_ready": lambda: L.crispy_rn_record_frames_ready(None),
        "crispy_rn_record_drain_device": lambda: L.crispy_rn_record_drain_device(None, 1, 1, p, 16, C.byref(n), None),
        "crispy_rn_record_drain": lambda: L.crispy_rn_record_drain(None, 1, 1, p, 16, C.byref(n)),
    }
    assert set(calls) == set(HANDLE_NAMES)
    for name, call in calls.items():
        assert call() == -1, name
        msg = L.crispy_last_error().decode()
        assert msg.startswith(name + ":") and "NULL handle" in msg, (name, msg)
    assert (n.value, mic.value, app.value) == (7, 7, 7) and not any(buf)
    # the pure one has no handle: a negative argument is its invalid call
    for args in ((-1, 0, 1), (0, -1, 1), (1152, 0, -1)):
        assert L.crispy_record_worker_plan(*args, None, None, None, None) == -1, args
        assert L.crispy_last_error().decode().startswith("crispy_record_worker_plan:")
    assert L.crispy_abi_version() == 6          # new entry points only: no struct grew, no argument changed meaning


def test_names_are_bound_and_declared():
    from crispy_amd import _native as N
    from crispy_amd.denoise import CaptureBuffers, DenoiseState
    L = _lib()
    hdr = open(os.path.join(ROOT, "include", "crispy_hip.h")).read()
    for name in NAMES:
        assert name in N.RN_SYMBOLS and name in N.ALL_SYMBOLS
        assert getattr(L, name).argtypes, name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    assert L.crispy_rn_record_frames_ready.restype is C.c_long and L.crispy_record_worker_plan.restype is C.c_long
    assert re.search(r"#define CRISPY_ABI_VERSION 6\b", hdr)
    for m in ("record_configure", "record_app_push", "level", "record_buffered", "record_frames_ready", "record_drain"):
        assert callable(getattr(DenoiseState, m)), m
    for m in ("push_mono", "push_mono_block", "drain_block"):          # the per-sample form stays, the block form is new
        assert callable(getattr(CaptureBuffers, m)), m
    assert N.REC_FRAME == RO.FRAME == 1152


# ---- 2 -------------------------------------------------------------------------------------------------------------
def _plan(L, mic_len, app_len, max_frames):
    room = max(1, min(max_frames, mic_len // RO.FRAME))
    mic_off, app_off = (C.c_long * room)(), (C.c_long * room)()
    mic_left, app_left = C.c_long(-9), C.c_long(-9)
    n = L.crispy_record_worker_plan(mic_len, app_len, max_frames, C.addressof(mic_off), C.addressof(app_off), C.byref(mic_left),
                                    C.byref(app_left))
    assert 0 <= n <= room, (mic_len, app_len, max_frames, n)
    return n, list(mic_off[:n]), list(app_off[:n]), mic_left.value, app_left.value


def test_worker_plan_equals_the_oracle_loop():
    L = _lib()
    F, D = RO.FRAME, RO.MAX_DESYNC
    edges = []
    for mf in (0, 1, 2, 1000):
        edges += [(F - 1, 0, mf), (F, 0, mf), (F, F - 1, mf), (F, F, mf), (5000, F - 1, mf), (5000, F, mf),
                  (3000 + D, 3000, mf), (3000 + D + 1, 3000, mf), (3000, 3000 + D, mf), (3000, 3000 + D + 1, mf),
                  (F + D, F, mf), (F + D + 1, F, mf), (F, F + D, mf), (F, F + D + 1, mf), (0, 0, mf), (0, 99999, mf),
                  (480000, 480000, mf), (480000, 0, mf), (F, 480000, mf)]
    rng = np.random.default_rng(20)
    cases = list(edges)
    for _ in range(2400):
        kind = rng.integers(4)
        mic = int(rng.integers(0, 30000))
        app = int(rng.integers(0, 30000)) if kind else int(np.clip(mic + rng.integers(-2500, 2500), 0, None))
        if kind == 3:
            mic, app = int(rng.integers(0, 480001)), int(rng.integers(0, 480001))
        cases.append((mic, app, int(rng.choice([0, 1, 2, 3, 7, 1 << 40]))))
    assert len(cases) >= 2000
    seen = dict(mic_trim=0, app_trim=0, zero_app=0, mixed=0, app_left_alone=0, limited=0)
    for mic, app, mf in cases:
        want_n, want_mic, want_app, want_ml, want_al, counts = RO.worker_plan(mic, app, mf)
        got = _plan(L, mic, app, mf)
        assert got == (want_n, want_mic, want_app, want_ml, want_al), (mic, app, mf)
        # count only: NULL arrays
        assert L.crispy_record_worker_plan(mic, app, mf, None, None, None, None) == want_n
        for k in counts:
            seen[k] += counts[k] > 0
        seen["limited"] += want_ml >= F
    assert all(v > 20 for v in seen.values()), seen          # every branch of the loop is taken by many cases
    # the figures of the loop's arithmetic, by hand: 5000 mic, 0 app -> trimmed to 2400, two frames of zeros, 96 left
    assert _plan(L, 5000, 0, 99) == (2, [2600, 3752], [-1, -1], 96, 0)
    # 1152 mic, 6000 app -> app trimmed to 3552, one mixed frame
    assert _plan(L, 1152, 6000, 99) == (1, [0], [2448], 0, 2400)


# ---- 3 -------------------------------------------------------------------------------------------------------------
def test_oracle_quantiser_gives_the_reference_vectors():
    """wav_writer_clamps_samples (recording.rs:483-504): 2.0, 1.5 -> 32767; -3.0, -1.5 -> -32767; and Rust's `as`."""
    q = RO.quantise(np.array([2.0, 1.5, -3.0, -1.5, 0.5, -0.5, 1.0, -1.0, 0.0, np.nan, np.inf, -np.inf], np.float32))
    assert q.tolist() == [32767, 32767, -32767, -32767, 16383, -16383, 32767, -32767, 0, 0, 32767, -32767]
    with np.errstate(invalid="ignore"):
        mixed = np.array([np.inf], np.float32) + np.array([-np.inf], np.float32)
    assert np.isnan(mixed[0]) and RO.quantise(mixed).tolist() == [0]
    assert RO.quantise(np.array([0.8], np.float32) + np.array([0.8], np.float32)).tolist() == [32767]
    assert RO.as_transcriber(np.array([16383, -32767], np.int16)).tolist() == [16383 / 32768, -32767 / 32768]
    # the downmix: one operation per Rust operation
    x = np.array([[0.1, 0.2, 0.7, -0.3, 0.25, 0.5]], np.float32)
    assert RO.downmix(x, 1).tobytes() == x.tobytes()
    f = np.float32
    assert RO.downmix(x, 2).tolist() == [[(f(0.1) + f(0.2)) / f(2), (f(0.7) + f(-0.3)) / f(2), (f(0.25) + f(0.5)) / f(2)]]
    assert RO.downmix(x, 3).tolist() == [[((f(0) + f(0.1) + f(0.2)) + f(0.7)) / f(3), ((f(0) + f(-0.3) + f(0.25)) + f(0.5)) / f(3)]]
    assert RO.level(np.array([[3.0, 4.0]], np.float32)).tolist() == [float(np.sqrt(f(12.5)))]
    # the deque with a cap: the oldest sample goes for each one that does not fit
    o = RO.RecordOracle(1, cap=5)
    o.push_mic(np.arange(4, dtype=np.float32)[None])
    o.push_mic(np.arange(4, 7, dtype=np.float32)[None])
    assert [float(r[0]) for r in o.mic] == [2, 3, 4, 5, 6] and o.mic_evictions == 2


# ---- 4 -------------------------------------------------------------------------------------------------------------
def _kernel_sections(isa):
    """{mangled name: its instructions} of an AMDGPU assembly listing."""
    out, cur = {}, None
    for line in isa.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            out[cur] = []
        elif cur and re.match(r"^\s+(s_endpgm)\b", line):
            out[cur].append(line)
            cur = None
        elif cur:
            out[cur].append(line)
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_record_kernels_have_no_scratch_and_contract_nothing(tmp_path):
    """The drain kernels hold no fused multiply-add at all.  The app and level kernels divide, and the level kernel takes a
    square root: correctly rounded, these are refinement sequences of v_fma_f32 on this hardware (v_div_scale / v_rcp / fma ... /
    v_div_fmas / v_div_fixup), so there the check is what the rule is for -- that no multiply was contracted with an add: the
    ISA is the same, instruction for instruction, when contraction is switched off for the whole compilation, and every fused
    operation of the app kernel lies inside a division sequence, of the level kernel behind the accumulation loop."""
    text = open(os.path.join(ROOT, "crispy_amd", "csrc", "Makefile")).read()
    assert "rn_record.hip" in re.search(r"^SRCS := (.*)$", text, re.M).group(1).split()
    flags = re.search(r"^CXXFLAGS \?= (.*)$", text, re.M).group(1).replace("$(ARCH)", "gfx950").split()
    assert not any("fast" in f or "contract" in f or "unsafe" in f or "approx" in f for f in flags), flags
    flags = [f for f in flags if f != "-fPIC" and not f.startswith("-W")]
    src = os.path.join(ROOT, "crispy_amd", "csrc", "rn_record.hip")

    def compile_to(asm, extra=()):
        out = subprocess.run([HIPCC, *flags, *extra, "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", src, "-o", str(asm)],
                             capture_output=True, text=True, timeout=600, cwd=os.path.dirname(src))
        assert out.returncode == 0, out.stderr[-2000:]
        return out.stderr, asm.read_text()

    remarks, isa = compile_to(tmp_path / "rec.s")
    res, cur = {}, None
    for line in remarks.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            res[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur:
            res[cur][m.group(1).strip()] = int(m.group(2))
    # the app pass, the level pass, and the drain in two formats x (16-byte stores, fallback)
    count = lambda word: sum(word in k for k in res)
    assert (count("rn_rec_app_kernel"), count("rn_level_kernel"), count("rn_rec_drain_kernel"), len(res)) == (1, 1, 4, 6), list(res)
    for name, r in res.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (name, r)
    sec = _kernel_sections(isa)
    assert set(sec) == set(res)
    for name, lines in sec.items():
        body = "\n".join(lines)
        if "rn_rec_drain_kernel" in name:
            assert not re.search(FMA, body), f"a fused multiply-add in {name}"
            assert "v_mul_f32" in body and "v_add_f32" in body and "v_cvt_i32_f32" in body, name       # x 32767, mic + app, as i16
        elif "rn_rec_app_kernel" in name:
            inside = False
            for ln in lines:
                if "v_div_scale_f32" in ln:
                    inside = True
                elif "v_div_fixup_f32" in ln:
                    inside = False
                elif re.search(FMA, ln):
                    assert inside, f"a fused multiply-add outside a division in {name}: {ln.strip()}"
            assert body.count("v_div_fixup_f32") >= 1 and "v_add_f32" in body, name
        else:
            first_div = next(i for i, ln in enumerate(lines) if "v_div_scale_f32" in ln)
            last_lds = max(i for i, ln in enumerate(lines) if re.search(r"\bds_(read|load)", ln))
            assert last_lds < first_div, name                      # the loop that reads the tile comes before the finish
            assert not re.search(FMA, "\n".join(lines[:first_div])), f"a fused multiply-add in the accumulation of {name}"
            assert "v_sqrt_f32" in body and "v_div_fixup_f32" in body, name
            assert "v_mul_f32" in "\n".join(lines[:first_div]) and "v_add_f32" in "\n".join(lines[:first_div]), name
    # no contraction anywhere: compiled with contraction off for everything, the listing is the same
    _, isa_off = compile_to(tmp_path / "rec_off.s", extra=("-ffp-contract=off",))
    strip = lambda s: [ln for ln in s.splitlines() if "__hip_cuid" not in ln]        # (a hash of the command line)
    assert strip(isa) == strip(isa_off), "rn_record.hip contracts a multiply-add somewhere"


# ---- 5 -------------------------------------------------------------------------------------------------------------
def test_wav_writer_writes_the_reference_spec(tmp_path):
    from crispy_amd.recording import CHANNELS, FRAME_SIZE, SAMPLE_RATE, WavWriter
    assert (SAMPLE_RATE, CHANNELS, FRAME_SIZE) == (48000, 2, 1152)
    rng = np.random.default_rng(5)
    q = rng.integers(-32767, 32768, size=3 * FRAME_SIZE).astype(np.int16)
    pcm = np.repeat(q, 2)                                    # a drained payload: L == R
    path = tmp_path / "rec.wav"
    w = WavWriter(path)
    w.write_frames(pcm[:2 * FRAME_SIZE])                     # one frame, then two
    w.write_frames(pcm[2 * FRAME_SIZE:].reshape(-1, 2))
    assert w.frames_written == 3 * FRAME_SIZE and w.finalize() == path
    with wave.open(str(path), "rb") as r:
        assert (r.getframerate(), r.getnchannels(), r.getsampwidth(), r.getnframes()) == (48000, 2, 2, 3 * FRAME_SIZE)
        back = np.frombuffer(r.readframes(r.getnframes()), dtype="<i2")
    assert back.tobytes() == pcm.astype("<i2").tobytes()
    # what run_transcription reads back: channel 0, / 32768
    assert (RO.as_transcriber(back[0::2]) == q.astype(np.float32) / np.float32(32768)).all()
    with pytest.raises(ValueError):
        WavWriter(tmp_path / "bad.wav").write_frames(np.zeros(4, np.float32))
