"""acm_chars_positions, acm_chars_records and the host path of acm_scan_chars under AddressSanitizer and UBSan: a
stand-alone C driver (tests/helpers/chars_driver.c) compiled together with the host C sources and run as a
program of its own, exactly as tests/test_words_sanitized.py builds its driver.  Nothing is loaded into Python
under a sanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chars_positions_records_and_scan_chars_host_path_under_asan_and_ubsan(tmp_path):
    csrc = os.path.join(ROOT, "aho-corasick-1975_amd", "csrc")
    exe = str(tmp_path / "chars_driver")
    # (the sanitizers' runtimes are linked statically: the program depends on no library load order)
    cmd = ["gcc", "-O1", "-g", "-std=c11", "-Wall", "-Wextra", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",
           "-I", os.path.join(ROOT, "include"), "-I", csrc, os.path.join(ROOT, "tests", "helpers", "chars_driver.c"),
           os.path.join(csrc, "acm_host.c"), os.path.join(csrc, "acm_flat.c"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks held" in r.stdout
