"""Standalone circular correlation on the host side: the drop-in names of reference utils/utils.py:285-301 and
models/operations_lp.py:58-68 (ccorr, pre_corr_op) exist with the reference's signatures, pre_corr_op stays out of the registries
and off the cell-zero compose path, and a CPU tensor is refused (there is no CPU fallback)."""
import importlib
import inspect

import pytest
import torch

import conftest  # noqa: F401  (puts the repository root on sys.path)


def test_names_import():
    from mr_gnas_amd import functional as K
    from mr_gnas_amd.operations_lp import ccorr, pre_corr_op  # noqa: F401
    from mr_gnas_amd.functional import ccorr as fccorr
    assert ccorr is fccorr is K.ccorr


def test_pre_corr_op_signatures_match_the_reference():
    from mr_gnas_amd.operations_lp import pre_corr_op
    assert list(inspect.signature(pre_corr_op.__init__).parameters) == ["self"]
    assert list(inspect.signature(pre_corr_op.forward).parameters) == ["self", "g", "src_emb", "hr"]
    op = pre_corr_op()
    assert list(op.state_dict()) == []


def test_pre_corr_op_is_an_operator_but_not_a_compose_op():
    from mr_gnas_amd import operations_lp as OPS
    assert issubclass(OPS.pre_corr_op, OPS._Operator)
    assert not issubclass(OPS.pre_corr_op, OPS._PreOp)
    assert not isinstance(OPS.pre_corr_op(), OPS._PreOp)


def test_registries_unchanged():
    from mr_gnas_amd import operations_lp as OPS
    assert OPS.PRE_OPS == ["pre_mult", "pre_sub", "pre_add"]
    assert list(OPS.MIXED_OPS) == ["pre_mult", "pre_sub", "pre_add", "f_zero", "f_identity", "f_dense", "f_dense_comp", "f_comp",
                                   "f_sparse", "f_sparse_comp", "f_dense_last", "f_sparse_last", "a_max", "a_mean", "a_sum"]
    assert "pre_corr" not in OPS.MIXED_OPS and "pre_corr" not in OPS.PRE_OPS


def test_cpu_tensors_raise():
    from mr_gnas_amd import _lib
    from mr_gnas_amd import functional as K
    from mr_gnas_amd.operations_lp import pre_corr_op
    a, b = torch.randn(4, 8), torch.randn(4, 8)
    with pytest.raises(_lib.MrgnasError):
        K.ccorr(a, b)
    with pytest.raises(_lib.MrgnasError):
        pre_corr_op()(None, a, b)


def test_switch_is_a_plain_attribute():
    from mr_gnas_amd.functional import switches as SW
    C = importlib.import_module("mr_gnas_amd.functional.ccorr")     # the package re-exports the function under the same name
    assert SW.CCORR_PATH is None
    assert C.matrix_ok(200) and C.matrix_ok(256) and not C.matrix_ok(7) and not C.matrix_ok(10) and not C.matrix_ok(48)
