"""CPU: the host-side C/C++ that parses untrusted files or does buffer arithmetic -- the FASTA reader and BED/TSV writers
(csrc/fasta_io.cpp), the work planner (csrc/plan.cpp) and the oracle (oracle/prf_oracle.c) -- built with
-fsanitize=address,undefined (make -C colab-repeat-finder_amd/csrc asan; gcc for the oracle) and driven through the CPU tests
of those parts in a child process with libasan preloaded ("Race detection / sanitizers").  GPU
AddressSanitizer is not available on the pool: the kernels are covered by the parity tests and the differential stress."""
import os
import subprocess
import sys

import pytest

from conftest import PKG, ROOT


def _runtime(name):
    path = subprocess.run(["gcc", f"-print-file-name={name}"], capture_output=True, text=True).stdout.strip()
    return path if os.path.isabs(path) and os.path.exists(path) else None


def test_host_code_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    asan = _runtime("libasan.so")
    if not asan:
        pytest.skip("no libasan.so next to gcc")
    subprocess.check_call(["make", "-C", os.path.join(PKG, "csrc"), "asan"], stdout=subprocess.DEVNULL)
    host_lib = os.path.join(PKG, "libprf_host_asan.so")
    oracle_lib = os.path.join(ROOT, "oracle", "libprf_oracle_asan.so")
    src = os.path.join(ROOT, "oracle", "prf_oracle.c")
    if not os.path.exists(oracle_lib) or os.path.getmtime(oracle_lib) < os.path.getmtime(src):
        subprocess.check_call(["gcc", "-O1", "-g", "-std=c11", "-fPIC", "-shared", "-Wall", "-fsanitize=address,undefined",
                               "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-o", oracle_lib, src])
    preload = " ".join([asan] + os.environ.get("LD_PRELOAD", "").split())   # the ASan runtime first, what was preloaded kept
    env = dict(os.environ, LD_PRELOAD=preload, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1",
               PRF_LIB=host_lib, PRF_LIB_HOST_ONLY="1", PRF_ORACLE_LIB=oracle_lib)
    # --rootdir: otherwise pytest roots the child at the common ancestor of its cwd (tmp_path) and the tests, a directory the
    # test user may not be allowed to list
    cmd = [sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", "--rootdir", ROOT,
           os.path.join(ROOT, "tests", "test_fasta_io.py"), os.path.join(ROOT, "tests", "test_plan.py"),
           os.path.join(ROOT, "tests", "test_oracle_golden.py")]
    res = subprocess.run(cmd, env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    report = res.stdout[-3000:] + res.stderr[-3000:]
    assert res.returncode == 0 and "AddressSanitizer" not in report and "runtime error" not in report, report
    assert " passed" in res.stdout
