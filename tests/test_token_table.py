"""The batch-token table, the pin guard and the two destroy sequences (dsp_slam_amd/csrc/batch_tokens.h) under host sanitizers.

tests/host/token_driver.cpp instantiates the header with stand-in handle and batch types: the single-threaded token rules, then 8 threads
registering, touching, batch-destroying and handle-destroying over 4 handles.  Every touch writes the batch and its handle, so a use after
free or an access without a pin is a sanitizer report.  A stand-alone program on the CPU: no GPU, no libdspgn, nothing preloaded."""
import pytest

import host_build


@pytest.mark.parametrize("sanitize", ["thread", "address,undefined"])
def test_token_table_under_sanitizer(tmp_path, sanitize):
    host_build.skip_on_gpu_machine()
    exe = host_build.compile_driver([host_build.HOST + "/token_driver.cpp"], sanitize, str(tmp_path / "token_driver"))
    out = host_build.run_driver([exe])
    assert out.startswith("ok:")
