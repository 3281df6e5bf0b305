"""The signing core as a stand-alone host program under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/sign_host_harness.cpp with its own main
(-DSIGN_HARNESS_MAIN) runs the edge scalars, the batched inversion at wave
sizes 1, 2, 63, 64 and with rejected lanes, the sc_muladd edge triples and
two RFC 8032 vectors through the whole chain.  An executable of its own:
nothing is preloaded and nothing is loaded into Python."""
import subprocess

from test_sign_host import build_harness


def test_sign_core_under_asan_ubsan(tmp_path):
    exe = tmp_path / "sign_san"
    build_harness(exe, ("-O0", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                        "-DSIGN_HARNESS_MAIN"))
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
