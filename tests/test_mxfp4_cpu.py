"""The MXFP4 family without a device: its planner's lines and the symbols of the built libraries."""
import pytest

from rag import _native as nat


@pytest.mark.parametrize("args, line", [
    ((64, 768, 128, 10_000_000, 256), "scan_mxfp4<ksteps=6,kp=128> streams=256 waves=4 lds=131072 + merge_sorted x2"),
    ((17, 384, 32, 4099, 256), "scan_mxfp4<ksteps=3,kp=32> streams=64 waves=2 lds=16384 + merge_sorted x2"),
    ((1, 100, 64, 53, 256), "scan_mxfp4<ksteps=1,kp=64> streams=1 waves=1 lds=16384 + merge_sorted x1"),
    ((64, 1024, 64, 1000, 8), "scan_mxfp4<ksteps=8,kp=64> streams=8 waves=4 lds=65536 + merge_sorted x1"),
])
def test_plan_lines(args, line):
    assert nat.mxfp4_plan_describe(*args) == line


@pytest.mark.parametrize("args", [(65, 384, 32, 100), (1, 1025, 32, 100), (1, 384, 48, 100), (1, 384, 32, 0)])
def test_plan_refuses(args):
    with pytest.raises(nat.NativeError):
        nat.mxfp4_plan_describe(*args)


def test_symbols_and_row_bytes():
    lib = nat.load()
    for name in ("crs_slab_append_mxfp4_f32", "crs_slab_write_rows_mxfp4_f32", "crs_mxfp4_topk", "crs_mxfp4_workspace_bytes"):
        assert hasattr(lib, name)
    assert hasattr(nat.ops(), "slab_write_mxfp4") and hasattr(nat.ops(), "mxfp4_topk")
    assert [nat.mxfp4_row_bytes(d) for d in (100, 384, 768, 1024)] == [80, 208, 416, 544]
    assert nat.mxfp4_slab_bytes(17, 768) == (2 * 16 * 384, 2 * 64 * 8)
