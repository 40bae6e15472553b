"""The wave-level idioms of crispy_amd/csrc are defined once (no GPU, reads the sources only).

wave_ops.h is the one home of the wave-local LDS sync, the LDS-only workgroup barrier, the DPP moves and row sums and the
__shfl_xor reductions; fft_lds.h of the complex helpers.  A second copy of one of them is how the bit-parity claims of
the kernels came to rest on copies edited in step (kernel conventions; NOTEBOOK.md 29)."""
import collections
import pathlib
import re

CSRC = pathlib.Path(__file__).resolve().parents[1] / "crispy_amd" / "csrc"
SOURCES = {p.name: p.read_text() for p in sorted(CSRC.iterdir()) if p.suffix in (".hip", ".h")}

# Sites left alone: file -> {the loop as written: (how often, kernel, why)}.  Each was replaced ALONE by shfl_sum / shfl_max
# and the kernel named came out of tools/isa_same.py (against the parent commit) as different code; a changed kernel is what
# that refactor did not allow itself.  First differing lines: NOTEBOOK.md 29.  Only single-value
# `for (off ...) v (+= | = fmaxf) __shfl_xor` loops are meant; any other such loop in any file fails the test.
SHUFFLE_LOOPS_LEFT_ALONE = {
    "whisper_attn.hip": {
        "for (int off = 32; off > 0; off >>= 1) mloc = fmaxf(mloc, __shfl_xor(mloc, off, 64));":
            (1, "attn_dec_kernel", "same instructions on other registers from line 614 on (v43 | v59)"),
        "for (int off = 32; off > 0; off >>= 1) lsum += __shfl_xor(lsum, off, 64);":
            (1, "attn_dec_kernel", "other register assignment, all three instances"),
        "for (int off = 8; off <= 32; off <<= 1) ls += __shfl_xor(ls, off, 64);":
            (2, "attn_dec_x16_kernel, attn_dec_x16g_kernel (mode 2's all-keys sum)", "the ds_bpermute address is scheduled elsewhere"),
    },
    "whisper_dec_fused.hip": {
        "for (int off = 8; off <= 32; off <<= 1) ls += __shfl_xor(ls, off, 64);":
            (1, "fd_attend in fused_self_kernel / fused_cross_kernel", "the ds_bpermute address is scheduled elsewhere"),
    },
    "whisper_dec_gemv.hip": {
        "for (int off = 16; off > 0; off >>= 1) acc[m] += __shfl_xor(acc[m], off, 64);":
            (1, "gemv_dec_kernel (half-wave tree, not one of the three ranges)", "147 of 165 instances on other registers"),
    },
}
SHUFFLE_LOOP = re.compile(r"for \(int off = \d+; off (?:>|<=) \d+; off (?:>>|<<)= 1\) "
                          r"([\w.\[\]]+) (?:\+= __shfl_xor\(\1, off, 64\)|= fmaxf\(\1, __shfl_xor\(\1, off, 64\)\));")


def files_with(needle):
    return {name for name, text in SOURCES.items() if needle in text}


def test_sources_found():
    assert {"wave_ops.h", "fft_lds.h", "rn_kernels.hip", "whisper_attn.hip"} <= set(SOURCES)


def test_lds_sync_and_fences_only_in_wave_ops():
    assert files_with("s_waitcnt(0xc07f)") == {"wave_ops.h"}
    assert files_with("__builtin_amdgcn_fence(") == {"wave_ops.h"}


def test_dpp_builtin_only_in_wave_ops_and_rn_wave_sums():
    assert "wave_ops.h" in files_with("__builtin_amdgcn_update_dpp")
    assert files_with("__builtin_amdgcn_update_dpp") <= {"wave_ops.h", "rn_wave_sums.h"}


def test_complex_multiply_defined_once():
    assert files_with("float2 cmul(") == {"fft_lds.h"}
    assert SOURCES["fft_lds.h"].count("float2 cmul(") == 1


def test_written_out_shuffle_reductions_only_where_recorded():
    for name, text in SOURCES.items():
        if name == "wave_ops.h":
            continue
        found = collections.Counter(m.group(0) for m in SHUFFLE_LOOP.finditer(text))
        allowed = {loop: n for loop, (n, _kernel, _why) in SHUFFLE_LOOPS_LEFT_ALONE.get(name, {}).items()}
        assert dict(found) == allowed, (name, dict(found))
