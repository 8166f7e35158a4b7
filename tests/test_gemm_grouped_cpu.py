"""CPU: host logic of the grouped Linear GEMM entry (vg_gemm_nt_f16x3_grouped, csrc/gemm_split.hip): workspace sizes,
the range of the group count and argument rejection -- all of it decided before any launch, so no device is needed."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from disentangle_mlp_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


FWD = (128, 2048, 16384)        # the discriminator's lth_features forward at batch 128: 16 tiles x 16 splits
DGRAD = (128, 16384, 2048)      # its data gradient: 128 tiles x 2 splits


def test_workspace_is_the_single_calls_per_group(lib):
    for shape in (FWD, DGRAD, (2048, 16384, 128), (130, 128, 1024), (5, 136, 64)):
        one = lib.vg_gemm_nt_f16x3_workspace_bytes(*shape)
        for g in (1, 2, 3):
            assert lib.vg_gemm_nt_f16x3_grouped_workspace_bytes(g, *shape) == g * one
    assert lib.vg_gemm_nt_f16x3_grouped_workspace_bytes(3, *FWD) == 3 * 16 * 128 * 2048 * 4
    assert lib.vg_gemm_nt_f16x3_grouped_workspace_bytes(2, *DGRAD) == 2 * 2 * 128 * 16384 * 4
    assert lib.vg_gemm_nt_f16x3_grouped_workspace_bytes(2, 130, 128, 1024) > 0      # the K split the GPU tests force
    assert lib.vg_gemm_nt_f16x3_grouped_workspace_bytes(2, 5, 136, 64) == 0         # ... and the shape without one


def test_group_count_outside_1_to_3_is_not_taken(lib):
    for g in (-1, 0, 4, 100):
        assert lib.vg_gemm_nt_f16x3_grouped_workspace_bytes(g, *FWD) == 0
    assert lib.vg_gemm_nt_f16x3_grouped_workspace_bytes(2, 128, 2048, 100) == 0     # K % 32: as the single entry


def _call(lib, groups, A, C, amax, B=0x2000, b_amax=0x3000, shape=FWD, strides=None, ws=0x100000, ws_bytes=1 << 40):
    """Never launches in these tests: every call is rejected on the host.  The pointers are made-up addresses."""
    arr = lambda v: (ctypes.c_void_p * len(v))(*v) if v is not None else None
    M, N, K = shape
    strides = strides or (K, 1, K, 1)
    return lib.vg_gemm_nt_f16x3_grouped(groups, arr(A), B, None, arr(C), M, N, K, *strides, arr(amax), b_amax, ws, ws_bytes,
                                        None)


def test_rejected_arguments(lib):
    A, C, S = [0x10000, 0x20000, 0x30000], [0x40000, 0x50000, 0x60000], [0x100, 0x200, 0x300]
    for g in (0, 4, -1):                                                  # G range
        assert _call(lib, g, A, C, S) == -1
    assert _call(lib, 2, None, C, S) == -1                                # NULL arrays
    assert _call(lib, 2, A, None, S) == -1
    assert _call(lib, 2, A, C, None) == -1
    assert _call(lib, 2, A, C, S, B=None) == -1
    assert _call(lib, 2, A, C, S, b_amax=None) == -1
    for bad in ([0x10000, None, 0x30000],):                               # a NULL inside the used part of an array
        assert _call(lib, 2, bad, C, S) == -1
        assert _call(lib, 2, A, bad, S) == -1
        assert _call(lib, 2, A, C, bad) == -1
    assert _call(lib, 2, A, C, S, shape=(128, 2048, 100)) == -1           # K % 32
    assert _call(lib, 2, A, C, S, shape=(0, 2048, 64)) == -1
    assert _call(lib, 2, A, C, S, strides=(16384, 2, 16384, 1)) == -1     # neither index contiguous
    assert _call(lib, 2, [0x10000, 0x20004, 0x30000], C, S) == -1         # 16-byte loads: every group's base aligned
    assert _call(lib, 2, A, C, S, B=0x2004) == -1
    # K split without room for every group's slabs: VG_ERR_WORKSPACE, and the single call's size is not enough for two
    one = lib.vg_gemm_nt_f16x3_workspace_bytes(*FWD)
    assert _call(lib, 2, A, C, S, ws=None, ws_bytes=0) == -2
    assert _call(lib, 2, A, C, S, ws_bytes=one) == -2
    assert _call(lib, 3, A, C, S, ws_bytes=3 * one - 1) == -2


def test_ops_wrapper_refuses_other_group_counts(lib):
    import torch
    from disentangle_mlp_amd import ops
    assert ops.GEMM_MAX_GROUPS == 3
    w = torch.zeros(4, 32)
    for n in (0, 4):
        with pytest.raises(RuntimeError, match="1..3 groups"):
            ops._gemm_nt_grouped([w] * n, w, None, [w] * n, 4, 4, 32, 32, 1, 32, 1, [w] * n, w)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.linear_fwd_grouped([w, w], w, None)
