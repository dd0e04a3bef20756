"""The canvas helper of kernel_ops.py can fail: a write into a padding column, into a guard row before the view and into a guard row
after it each make untouched() raise, a write inside the view does not.  Runs without a GPU."""
import pytest
import torch

import kernel_ops as ops

BF = torch.bfloat16


@pytest.mark.parametrize("dtype,fill", [(BF, ops.CANARY), (BF, ops.NAN), (torch.uint8, ops.CANARY), (torch.uint8, ops.NAN),
                                         (torch.float32, ops.CANARY)])
def test_untouched_sees_every_region(dtype, fill):
    rows, cols, ld = 5, 13, 24
    raw_t = ops._RAW[dtype]

    def fresh():
        return ops.canvas(rows, cols, ld, dtype, fill)

    cv = fresh()
    assert cv.view.shape == (rows, cols) and cv.view.stride() == (ld, 1)
    assert cv.guard >= ops.TILE_ROWS and cv.buf.shape == (2 * cv.guard + rows, ld)
    assert cv.view.data_ptr() == cv.buf.data_ptr() + cv.guard * ld * cv.buf.element_size()
    assert cv.untouched() and cv.untouched(whole=True)
    # inside the view: allowed (and seen by whole=True only)
    cv.view.view(raw_t)[2, 3] = 1
    cv.view.view(raw_t)[rows - 1, cols - 1] = 1
    assert cv.untouched()
    with pytest.raises(AssertionError, match="view"):
        cv.untouched(whole=True)
    # one element in each region outside it
    for r, c, where in [(cv.guard + 2, cols, "padding columns"), (cv.guard + rows - 1, ld - 1, "padding columns"),
                        (cv.guard - 1, ld - 1, "before the view"), (0, 0, "before the view"), (cv.guard - 1, 0, "before the view"),
                        (cv.guard + rows, 0, "after the view"), (2 * cv.guard + rows - 1, ld - 1, "after the view")]:
        cv = fresh()
        cv.raw[r, c] = 1
        with pytest.raises(AssertionError, match=where):
            cv.untouched()
    # the comparison is on bit patterns: -0.0 over a 0.0 fill, another NaN payload over a NaN fill
    cv = ops.canvas(rows, cols, ld, BF, 0)
    cv.buf[cv.guard, cols] = -0.0
    with pytest.raises(AssertionError):
        cv.untouched()
    cv = ops.canvas(rows, cols, ld, BF, ops.NAN)
    cv.raw[cv.guard, cols] = 0x7FC1
    with pytest.raises(AssertionError):
        cv.untouched()


def test_fills_and_load():
    nan = ops.canvas(4, 8, 16, BF, ops.NAN)
    assert nan.buf.isnan().all() and set(nan.raw[:2, 0].tolist()) == {0x7FC0, -1}
    assert ops.canvas(4, 8, 16, torch.uint8, ops.NAN).buf.view(torch.float8_e4m3fn).float().isnan().all()
    can = ops.canvas(4, 8, 16, BF, ops.CANARY)
    assert not can.buf.isnan().any() and (can.raw == 0x5A5A).all()
    assert (ops.canvas(4, 8, 16, torch.float32, ops.CANARY).raw == 0x5A5A5A5A).all()
    # operand values loaded into the view belong to the expected state: untouched(whole=True) then guards them too
    x = torch.randn(4, 8).to(BF)
    v = nan.load(x)
    assert torch.equal(v, x) and nan.untouched(whole=True) and nan.buf[:nan.guard].isnan().all() and nan.buf[nan.guard:nan.guard + 4, 8:].isnan().all()
    v[1, 1] += 1
    assert nan.untouched()
    with pytest.raises(AssertionError):
        nan.untouched(whole=True)


def test_guards_cover_a_swapped_pitch():
    """guard_rows_for: the rows of the view rounded up by one more tile and walked at the widest pitch of the call stay inside"""
    for rows, ld, widest in [(130, 136, 216), (1001, 152, 1011), (5, 8200, 8208), (1, 8, 8), (300, 208, 216)]:
        g = ops.guard_rows_for(rows, ld, widest)
        assert g >= ops.TILE_ROWS and (rows + g) * ld >= (rows + ops.TILE_ROWS) * max(ld, widest)
    cv = ops.canvas(3, 8, 16, BF, ops.CANARY, guard_rows=ops.guard_rows_for(3, 16, 64))
    assert cv.guard == ops.guard_rows_for(3, 16, 64) > ops.TILE_ROWS
    with pytest.raises(AssertionError):
        ops.canvas(3, 8, 16, BF, ops.CANARY, guard_rows=8)
