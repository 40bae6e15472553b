"""Confidence entry points, host side (no GPU): the six names in the header, the Python binding and the Rust crate; the ABI
version and the mirrored structs unchanged (new entry points only); the accessors' argument checks; the new kernel file's
private segment."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
HEADER = os.path.join(ROOT, "include", "crispy_hip.h")
NAMES = ("crispy_asr_set_confidence", "crispy_asr_result_token_probs", "crispy_asr_result_word_probs",
         "crispy_asr_result_language_probs", "crispy_asr_detect_language_probs_device", "crispy_asr_token_probs_device")


def _lib():
    from crispy_amd import _native as N
    return N, N.lib()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_the_six_names_are_declared_bound_and_mirrored():
    N, L = _lib()
    hdr = _header()
    rs = open(os.path.join(ROOT, "bindings", "rust", "crispy-hip-sys", "src", "lib.rs")).read()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in N.ALL_SYMBOLS and hasattr(L, name) and getattr(L, name).argtypes, name
        assert re.search(r"pub fn %s\(" % name, rs), name
    assert re.search(r"pub const CRISPY_ABI_VERSION: c_int = 6;", rs)


def test_abi_version_is_still_6():
    _, L = _lib()
    assert L.crispy_abi_version() == 6          # new entry points only: no struct grew
    assert re.search(r"#define CRISPY_ABI_VERSION 6\b", open(HEADER).read())


def _c_sizeof(struct_name):
    """sizeof of a struct of the header, from its text: every field is an int / float (4 bytes), a size_t or a pointer (8),
    each aligned to its size, the struct padded to its widest member (the x86-64 / LP64 rules the library is built under)."""
    m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct_name, struct_name), _header(), flags=re.S)
    assert m, struct_name
    off, widest = 0, 1
    for decl in (d.strip() for d in m.group(1).split(";")):
        if not decl:
            continue
        ty, names = re.match(r"((?:const )?(?:unsigned )?\w+)\s*(.*)", decl, flags=re.S).groups()
        for nm in (n.strip() for n in names.split(",")):
            if "*" in nm:
                size = 8
            elif ty.split()[-1] in ("int", "float", "unsigned"):
                size = 4
            elif ty.split()[-1] in ("size_t", "long", "double"):
                size = 8
            else:
                raise AssertionError(f"{struct_name}: field '{decl}' of a type this test does not know")
            off = (off + size - 1) // size * size + size
            widest = max(widest, size)
    return (off + widest - 1) // widest * widest


@pytest.mark.parametrize("c_name,py_name", [("crispy_asr_opts", "AsrOpts"), ("crispy_asr_result", "AsrResult"), ("crispy_asr_word", "AsrWord")])
def test_mirrored_structs_keep_their_size(c_name, py_name):
    N, _ = _lib()
    assert C.sizeof(getattr(N, py_name)) == _c_sizeof(c_name)
    # ... and nothing of the new feature sits in them
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (c_name, c_name), _header(), flags=re.S).group(1)
    assert not re.search(r"\b(plog|p_forced|prob|probs|confidence)\b", body), c_name


def test_accessors_reject_null_without_a_device():
    N, L = _lib()
    FP = C.POINTER(C.c_float)
    p, q, n = FP(), FP(), C.c_int()
    fake = C.create_string_buffer(256)            # never read: every call below fails on a NULL before it looks at the result
    bad = int(re.search(r"CRISPY_ERR_INVALID_ARG = (-?\d+)", open(HEADER).read()).group(1))
    assert L.crispy_asr_result_token_probs(None, C.byref(p), C.byref(q), C.byref(n)) == bad
    assert b"NULL" in L.crispy_last_error()
    assert L.crispy_asr_result_token_probs(fake, None, C.byref(q), C.byref(n)) == bad
    assert L.crispy_asr_result_token_probs(fake, C.byref(p), None, C.byref(n)) == bad
    assert L.crispy_asr_result_token_probs(fake, C.byref(p), C.byref(q), None) == bad
    assert L.crispy_asr_result_word_probs(None, C.byref(p), C.byref(n)) == bad
    assert L.crispy_asr_result_word_probs(fake, None, C.byref(n)) == bad
    assert L.crispy_asr_result_word_probs(fake, C.byref(p), None) == bad
    assert L.crispy_asr_result_language_probs(None, C.byref(p), C.byref(n)) == bad
    assert L.crispy_asr_result_language_probs(fake, None, C.byref(n)) == bad
    assert L.crispy_asr_result_language_probs(fake, C.byref(p), None) == bad
    assert L.crispy_asr_set_confidence(None, 1) == bad
    assert L.crispy_asr_detect_language_probs_device(None, None, 1, None, None) == bad
    assert L.crispy_asr_token_probs_device(None, None, 1, None, None, 1, 1, None) == bad


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_confidence_kernels_use_no_private_segment(tmp_path):
    """whisper_conf.hip with the shipped flags: both kernels are there, wave64, and the code-object metadata gives every
    kernel a private segment (scratch) of 0 bytes."""
    from tests.test_build_resources import CGFLAGS
    src = os.path.join(ROOT, "crispy_amd", "csrc", "whisper_conf.hip")
    asm = tmp_path / "conf.s"
    out = subprocess.run([HIPCC, *CGFLAGS, "--cuda-device-only", "-S", src, "-o", str(asm)], capture_output=True, text=True,
                         timeout=600, cwd=os.path.dirname(src))
    assert out.returncode == 0, out.stderr[-2000:]
    text = asm.read_text()
    meta = text[text.index("amdhsa.kernels:"):]
    kernels = re.findall(r"\.name:\s+(\S+)", meta)
    sizes = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", meta)]
    waves = [int(v) for v in re.findall(r"\.wavefront_size:\s+(\d+)", meta)]
    assert any("tok_logprob_kernel" in k for k in kernels) and any("lang_probs_kernel" in k for k in kernels), kernels
    assert len(sizes) == len(waves) == 2 and sizes == [0, 0] and waves == [64, 64], (kernels, sizes, waves)
