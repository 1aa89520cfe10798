"""The snapshot blob's Writer and Reader (siddhi_amd/csrc/snap_io.h) on the host: what every Writer
call wrote reads back equal with zero padding; every truncated length throws "snapshot truncated"
without reading past the end; counts near SIZE_MAX do not wrap; need() throws its message."""
import pytest

from snap_io_host import CHECKS, run


@pytest.mark.parametrize("check", CHECKS)
def test_snap_io(check):
    assert run(check) == (0, "")
