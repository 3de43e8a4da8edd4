"""The C ABI traffic of the C++ host layer for the seven factor kinds, without a GPU: host/test/factor_trace.cpp drives the public API
of host/bundle_adjustment.cpp over a recording stand-in for the device library (host/test/fake_cuba_hip.cpp) -- every kind added, added
twice, removed, emptied, swept away with its vertex, refused, cleared -- and prints every call with its arguments, every chi2 it reads
back and every exception.  tests/golden/host_factor_calls.txt is that output as recorded from the host layer of commit 4148c40, before
the kinds were folded into one description each: order and content of the calls are the contract, byte for byte."""
import os
import subprocess

from conftest import ROOT

HOST = os.path.join(ROOT, "cuda-bundle-adjustment_amd", "host")
GOLDEN = os.path.join(ROOT, "tests", "golden", "host_factor_calls.txt")


def test_host_layer_factor_calls_match_the_record():
    subprocess.check_call(["make", "-C", HOST, "-s", "factor_trace"])
    env = {k: v for k, v in os.environ.items() if not k.startswith("CUBA_")}      # (the host layer turns CUBA_HIP_* variables into calls)
    out = subprocess.run([os.path.join(HOST, "factor_trace")], capture_output=True, env=env, timeout=60)
    assert out.returncode == 0, out.stdout[-2000:].decode() + out.stderr[-2000:].decode()
    want = open(GOLDEN, "rb").read()
    if out.stdout != want:
        got_lines, want_lines = out.stdout.decode().splitlines(), want.decode().splitlines()
        k = next((i for i, (a, b) in enumerate(zip(got_lines, want_lines)) if a != b), min(len(got_lines), len(want_lines)))
        context = "\n".join(m for m in want_lines[:k] if m.startswith("=="))[-300:]
        raise AssertionError(f"first difference in line {k + 1} ({len(got_lines)} lines, recorded {len(want_lines)}), after\n{context}\n"
                             f"got:      {got_lines[k][:400] if k < len(got_lines) else '<end>'}\n"
                             f"recorded: {want_lines[k][:400] if k < len(want_lines) else '<end>'}")
