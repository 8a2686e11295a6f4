"""TurnByTurn.tunes without a GPU: the C-ABI entry point is exported and bound, the Python constants are the header's, the
host-callable logic of csrc/chx_tunes_dev.h passes its stand-alone check, and argument errors are raised before any device work
(before the "GPU only" error of CPU tensors)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_constant(name: str) -> int:
    text = open(os.path.join(ROOT, "include", "chx.h")).read()
    return int(re.search(rf"#define {name} (\d+)", text).group(1))


def _records(R=32, K=4, lead=(), record_every=None, dtype=torch.float32):
    """A hand-built TurnByTurn of CPU tensors: R records of K rows."""
    import cheetah_amd as ca
    from cheetah_amd.particles.turns import NUM_SUMS

    return ca.TurnByTurn(None, torch.zeros(*lead, K + 3, dtype=torch.int32), torch.arange(1, R + 1) * (record_every or 1),
                         torch.zeros(R, *lead, NUM_SUMS, dtype=torch.float64), torch.zeros(R, *lead, K, 7, dtype=dtype),
                         record_every=record_every)


def test_tunes_symbol_exported_and_bound():
    import cheetah_amd._lib as L
    import cheetah_amd._ops  # noqa: F401  (adds the signature)

    lib = L.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    exported = set(re.findall(r" T (chx_[a-z0-9_]+)", out))
    assert "chx_tunes" in exported
    assert "chx_tunes" in L.SIGNATURES
    assert lib.chx_tunes.argtypes == L.SIGNATURES["chx_tunes"][1] and lib.chx_tunes.restype is ctypes.c_int
    assert lib.chx_abi_version() == 9


def test_python_constants_are_the_headers():
    import cheetah_amd as ca

    assert ca._ops.TUNES_T_MIN == _header_constant("CHX_TUNES_T_MIN") == 8
    assert ca._ops.TUNES_T_MAX == _header_constant("CHX_TUNES_T_MAX") == 4096
    assert callable(ca.TurnByTurn.tunes) and callable(ca.TurnByTurn.tune_diffusion)


def test_tunes_logic_on_the_host(tmp_path):
    """csrc/chx_tunes_dev.h (the coarse transform's items and positions, the choice of the peak and its bracket, the safeguarded
    Newton step, the edge cases) against long-double evaluations, compiled for the host only (no GPU, no HIP runtime call)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = tmp_path / "tunes_check"
    subprocess.run([hipcc, "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "cheetah_amd", "csrc"),
                    "-o", str(exe), os.path.join(ROOT, "tests", "host", "tunes_check.hip")], check=True, capture_output=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    for part in ("grid", "transform", "path", "root", "edges", "all"):
        assert f"{part}: ok" in out.stdout, out.stdout


def test_invalid_arguments_are_refused_before_any_launch():
    import cheetah_amd._lib as L
    import cheetah_amd._ops  # noqa: F401

    lib = L.lib()
    buf = (ctypes.c_double * 64)()                 # host memory standing in for pointers that must never be dereferenced
    p = ctypes.addressof(buf)

    def call(probe=p, R=64, S=3, r0=0, T=16, columns=3, dtype=1, nu=p, amp=p):
        return lib.chx_tunes(probe, None, R, S, r0, T, r0 + T, columns, dtype, nu, amp, None)

    assert call(probe=None) == -1
    assert call(nu=None) == -1
    assert call(amp=None) == -1
    assert call(R=0) == -1
    assert call(S=0) == -1
    assert call(r0=-1) == -1
    assert call(T=7) == -1
    assert call(T=4097, R=8192) == -1
    assert call(R=64, r0=49, T=16) == -1           # the window ends one record behind the last
    assert call(columns=0) == -1
    assert call(columns=8) == -1
    assert call(dtype=2) == -2


def test_records_are_needed():
    import cheetah_amd as ca
    from cheetah_amd.particles.turns import NUM_SUMS

    tbt = ca.TurnByTurn(None, torch.zeros(5, dtype=torch.int32), torch.arange(1, 33), torch.zeros(32, NUM_SUMS, dtype=torch.float64))
    with pytest.raises(ValueError, match="record_first"):
        tbt.tunes()
    with pytest.raises(ValueError, match="record_first"):
        tbt.tune_diffusion()


@pytest.mark.parametrize("R,kwargs,match", [
    (32, {"planes": ("x", "z")}, "planes"),
    (32, {"planes": ("x", "x")}, "planes"),
    (32, {"planes": ()}, "planes"),
    (32, {"planes": ("X",)}, "planes"),
    (7, {}, "record_every"),
    (32, {"num_records": 7}, "record_every"),
    (32, {"first_record": 25}, "record_every"),                 # 7 records are left
    (5000, {}, "record_every"),
    (5000, {"num_records": 4097}, "windows"),
    (32, {"first_record": 20, "num_records": 16}, "outside"),
    (32, {"first_record": -1, "num_records": 16}, "outside"),
    (32, {"num_records": 33}, "outside"),
])
def test_argument_errors_come_before_the_gpu_check(R, kwargs, match):
    with pytest.raises(ValueError, match=match):
        _records(R=R).tunes(**kwargs)


def test_tune_diffusion_takes_two_halves():
    with pytest.raises(ValueError, match="record_every"):       # 15 // 2 = 7 records per half
        _records(R=15).tune_diffusion()
    with pytest.raises(RuntimeError, match="GPU only"):
        _records(R=16).tune_diffusion()


@pytest.mark.parametrize("lead", [(), (2,)])
def test_cpu_records_are_refused(lead):
    with pytest.raises(RuntimeError, match="GPU only"):
        _records(lead=lead).tunes()
    with pytest.raises(RuntimeError, match="GPU only"):
        _records(lead=lead, record_every=3).tunes(planes="tau", first_record=8, num_records=8)
