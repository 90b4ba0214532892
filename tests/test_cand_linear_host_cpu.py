"""The grouped candidate-Linear entry points (ABI 22, csrc/cand_linear.hip) without a GPU: argument validation happens before any
launch, the shape queries are host functions."""
import ctypes

from mr_gnas_amd import _lib

P = ctypes.c_void_p
NEW = ("mrg_cand_linear_fwd", "mrg_cand_linear_bwd_input", "mrg_cand_linear_colsum_blocks", "mrg_cand_linear_workspace_bytes")


def arr(*vals):
    return (ctypes.c_void_p * len(vals))(*vals)


def test_the_library_reports_abi_22_and_declares_the_entry_points():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 23 and lib.mrg_abi_version() == 23
    for name in NEW:
        assert name in _lib.SIGNATURES and name in _lib.declared_symbols() and hasattr(lib, name)


def test_argument_errors_without_gpu():
    lib = _lib.load()
    ok = arr(16, 32, 48, 64)
    fwd = lambda n, X, W, b, Y, rows, D, ws=None, cs=None, nb=0: lib.mrg_cand_linear_fwd(n, X, W, b, Y, ws, rows, D, None, cs, nb)
    bwd = lambda n, G, W, X, rows, D, ws=None: lib.mrg_cand_linear_bwd_input(n, G, W, X, ws, rows, D, None)
    # NULL arrays, or a NULL member pointer -> -1
    assert fwd(2, None, ok, ok, ok, 8, 64) == -1
    assert fwd(2, ok, None, ok, ok, 8, 64) == -1
    assert fwd(2, ok, ok, ok, None, 8, 64) == -1
    assert fwd(2, arr(16, None), ok, ok, ok, 8, 64) == -1
    assert bwd(2, None, ok, ok, 8, 64) == -1 and bwd(2, ok, ok, arr(16, None), 8, 64) == -1
    # n outside 1..4, non-positive sizes -> -2
    for n in (0, 5, -1):
        assert fwd(n, ok, ok, ok, ok, 8, 64) == -2 and bwd(n, ok, ok, ok, 8, 64) == -2
    assert fwd(2, ok, ok, ok, ok, -1, 64) == -2 and fwd(2, ok, ok, ok, ok, 8, 0) == -2 and bwd(2, ok, ok, ok, 8, -4) == -2
    # shapes without a grouped form -> MRG_E_SHAPE (the host falls back to the per-member entry points)
    for D in (6, 12, 18, 132, 200):
        assert fwd(1, ok, ok, ok, ok, 8, D) == -2 and bwd(1, ok, ok, ok, 8, D) == -2
    assert fwd(1, arr(20), ok, ok, ok, 8, 64) == -2                   # a row pointer that is not 16-byte aligned
    # the bias array, or any entry of it, may be NULL; rows == 0 -> 0 (nothing to do, nothing launched)
    assert fwd(4, ok, ok, None, ok, 0, 64) == 0 and fwd(3, ok, ok, arr(16, None, 16), ok, 0, 128) == 0 and bwd(4, ok, ok, ok, 0, 16) == 0
    # column sums sized for another number of partials -> MRG_E_SHAPE
    assert fwd(1, ok, ok, ok, ok, 300, 64, cs=P(64), nb=1) == -2


def test_workspace_rule():
    """A missing workspace is MRG_E_WORKSPACE (-4) exactly when mrg_cand_linear_workspace_bytes asks for one.  This matrix core stages
    the weight in LDS and asks for none at any shape, so a NULL workspace is accepted everywhere."""
    lib = _lib.load()
    for n in (1, 4):
        for D in (16, 64, 128):
            assert lib.mrg_cand_linear_workspace_bytes(n, D) == 0
    assert b"workspace" in lib.mrg_error_string(-4)


def test_colsum_blocks():
    lib = _lib.load()
    blocks = lib.mrg_cand_linear_colsum_blocks
    assert blocks(40003, 6) == 0 and blocks(40003, 200) == 0 and blocks(40003, 132) == 0 and blocks(40003, 12) == 0
    assert blocks(0, 64) == 0
    for D in (16, 20, 64, 100, 128):
        assert blocks(1, D) == 1 and blocks(256, D) == 1 and blocks(257, D) == 2 and blocks(40003, D) == 157
    # the partial buffer stays a small fraction of one [rows, D] tensor (256-row workgroups: 1.6 %)
    assert blocks(40003, 64) * 2 * 64 * 8 <= 0.02 * 40003 * 64 * 4
