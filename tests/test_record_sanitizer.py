"""AddressSanitizer + UndefinedBehaviorSanitizer over csrc/vnl_record.hip (host code only): the stand-alone driver
tests/hostsim/record_sanitizer_main.cpp -- its own main, the entry and the kernel compiled for the host against
tests/hostsim/stub, synthetic buffers at their exact sizes -- built with -fsanitize=address,undefined and run as a plain
executable.  Nothing is loaded into Python."""
import os
import subprocess

import helpers as H


def test_record_entry_and_kernel_are_clean_under_asan_and_ubsan():
    hostsim = os.path.join(H.ROOT, "tests", "hostsim")
    exe = os.path.join(hostsim, "_build", "record_sanitizer")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    # (the runtimes linked statically: the executable carries them, whatever else the process environment loads first)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",
                           "-fno-omit-frame-pointer", "-DVNL_REAL=float", "-I" + os.path.join(hostsim, "stub"),
                           os.path.join(hostsim, "record_sanitizer_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    assert "record ok" in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
