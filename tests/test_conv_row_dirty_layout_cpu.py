"""CPU: the row_dirty array of a persistent convolution output (include/pnx.h): [flag bytes][pad][uint32 written masks][pad], stated once as a carve
in csrc/conv_tile.h and sized by pnx_conv3x3_row_dirty_bytes.  ops.conv3x3_workspace allocates exactly that and hands out the flags as the
(B, ho, segs) uint8 view at offset 0 -- the array every launch-plan pointer and every tile list points at, so the launch schedule that
tests/test_fused_schedule_cpu.py pins is unchanged."""
import pytest
import torch

SHAPES = [(1, 1, 1), (2, 37, 70), (2, 19, 35), (12, 1440, 1440), (12, 720, 720), (12, 360, 360), (12, 180, 180), (1, 8, 256), (3, 5, 257)]


def _up(n):
    return (n + 255) // 256 * 256


@pytest.mark.parametrize("shape", SHAPES)
def test_workspace_is_the_carved_array(shape):
    from pillarnext_amd import _lib, ops

    B, ho, wo = shape
    segs = (wo + 31) // 32
    n = B * ho * segs
    need = int(_lib.lib().pnx_conv3x3_row_dirty_bytes(B, ho, wo))
    assert need == ops.row_dirty_bytes(B, ho, wo) == _up(n) + _up(4 * n)          # flags, then one aligned uint32 per segment
    if B * ho * wo > 1 << 20:   # the benchmark's stages: the size alone (the output buffer would be gigabytes)
        return
    y, flags = ops.conv3x3_workspace(B, 64, ho, wo, "cpu")
    assert flags.dtype == torch.uint8 and tuple(flags.shape) == (B, ho, segs) and flags.is_contiguous()
    assert flags.storage_offset() == 0 and flags.untyped_storage().nbytes() == need
    assert tuple(y.shape) == (B, 64, ho, wo) and not flags.any() and not y.any()
    written = ops.row_dirty_written(flags, wo)
    assert written.dtype == torch.int32 and tuple(written.shape) == (B, ho, segs) and not written.any()
    assert written.untyped_storage().data_ptr() == flags.untyped_storage().data_ptr()
    assert written.storage_offset() * 4 == _up(n) and written.data_ptr() % 256 == flags.data_ptr() % 256
    written[-1, -1, -1] = -1                                                       # the last word lies inside the array, behind every flag
    assert not flags.any() and int(written.view(torch.uint8).sum()) == 4 * 255


def test_empty_shapes_and_old_size_arrays():
    from pillarnext_amd import _lib, ops
    from pillarnext_amd._lib import PnxError

    L = _lib.lib()
    assert L.pnx_conv3x3_row_dirty_bytes(0, 8, 8) == 0 and L.pnx_conv3x3_row_dirty_bytes(1, -1, 8) == 0
    old = torch.zeros((2, 19, 3), dtype=torch.uint8)                               # the flags alone: what the array was before the written masks
    with pytest.raises(PnxError, match="row_dirty"):
        ops.row_dirty_written(old, 70)
    with pytest.raises(PnxError, match="row_dirty"):
        ops._row_dirty_check(old, 2, 19, 70)                                       # what conv3x3_masked asks before it launches
    ops._row_dirty_check(ops.conv3x3_workspace(2, 64, 19, 70, "cpu")[1], 2, 19, 70)
