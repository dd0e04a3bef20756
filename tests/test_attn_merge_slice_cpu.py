"""The partition of a kv head's n_rep x D merged attention outputs over the head's context splits in the one-launch decode block
(attn_merge_slice in csrc/o3v_attn_decode_body.h, the function the kernel itself calls), through the C ABI: no GPU needed."""
import ctypes as C

import pytest

from open_o3_video_amd import _lib


@pytest.fixture(scope="module")
def merge_slice():
    fn = C.CDLL(_lib.LIB_PATH).o3v_attn_merge_slice
    fn.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    fn.restype = C.c_int
    return fn


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("n_rep", range(1, 9))
def test_slices_partition_the_outputs_on_the_8_element_grid(merge_slice, n_rep, D):
    n_out = n_rep * D
    b, c = C.c_int(), C.c_int()
    for nsplit in range(1, 65):
        end = 0   # the slices are disjoint, ascending and cover [0, n_out) exactly iff each begins where the one before it ended
        for split in range(nsplit):
            assert merge_slice(n_out, nsplit, split, C.byref(b), C.byref(c)) == _lib.OK
            assert b.value % 8 == 0 and c.value % 8 == 0 and c.value >= 0, (nsplit, split, b.value, c.value)
            assert b.value == end, (nsplit, split, b.value, end)
            end = b.value + c.value
            assert end <= n_out
        assert end == n_out, (nsplit, end)
        if nsplit == 1:
            assert (b.value, c.value) == (0, n_out)   # one workgroup merges the whole head group


def test_every_load_and_the_lds_of_the_merge_fit(merge_slice):
    """What the kernel sizes by the partition: two 16-byte loads per thread (256 threads) cover count / 4 quads x nsplit splits, and
    the [nsplit][count] fp32 partials end in front of the split weights (byte 33536 of the block's LDS)."""
    b, c = C.c_int(), C.c_int()
    for n_rep in range(1, 9):
        for nsplit in range(1, 65):
            for split in range(nsplit):
                merge_slice(n_rep * 128, nsplit, split, C.byref(b), C.byref(c))
                assert (c.value // 4) * nsplit <= 2 * 256
                assert c.value * nsplit * 4 <= 33536


def test_rejects_bad_arguments(merge_slice):
    b, c = C.c_int(), C.c_int()
    for n_out, nsplit, split in [(0, 1, 0), (100, 1, 0), (128, 0, 0), (128, 65, 0), (128, 4, 4), (128, 4, -1)]:
        assert merge_slice(n_out, nsplit, split, C.byref(b), C.byref(c)) == _lib.ERR_ARG
    assert merge_slice(128, 1, 0, None, C.byref(c)) == _lib.ERR_ARG
