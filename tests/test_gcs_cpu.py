"""Checks the checker of tests/test_gcs_gpu.py on the CPU (tests/gcs_ref.py): the FFT references against the double sum,
the convolution against its mirrored-correlation identity (the one the kernels' CCONV mode is built on), and the a-priori
bound against a float32 emulation of the kernels' summation order -- the bound must hold for that arithmetic, and it must
be able to fail: one dropped product in a list of one element lands outside it."""
import pytest
import torch

import conftest  # noqa: F401  (puts the repository root on sys.path)
import gcs_ref as R


@pytest.mark.parametrize("D", [1, 2, 7, 16, 50, 100, 200, 256])
def test_references_agree(D):
    gen = torch.Generator().manual_seed(D)
    a, b = torch.randn(33, D, generator=gen, dtype=torch.float64), torch.randn(33, D, generator=gen, dtype=torch.float64)
    for fft, conv in ((R.corr64, False), (R.conv64, True)):
        d = R.direct64(a, b, conv=conv)
        assert float((fft(a, b) - d).abs().max()) <= 1e-10 * float(d.abs().max())


@pytest.mark.parametrize("D", [1, 7, 16, 100, 200])
def test_conv_is_mirrored_corr(D):
    """conv(x, y)[k] = corr(x, z)[(D - k) % D] with z[m] = y[(D - m) % D]."""
    gen = torch.Generator().manual_seed(100 + D)
    x, y = torch.randn(9, D, generator=gen, dtype=torch.float64), torch.randn(9, D, generator=gen, dtype=torch.float64)
    mirror = (D - torch.arange(D)) % D
    want = R.corr64(x, y[:, mirror])[:, mirror]
    got = R.conv64(x, y)
    assert float((got - want).abs().max()) <= 1e-10 * float(want.abs().max())
    assert float((R.direct64(x, y, conv=True) - R.direct64(x, y[:, mirror])[:, mirror]).abs().max()) <= 1e-12 * float(want.abs().max())


def test_cases_have_the_promised_segments():
    c = R.mixed(16)
    L = torch.bincount(c["seg"], minlength=c["nseg"])
    assert c["nseg"] == 300 and int(L.max()) == 9000 and int((L == 0).sum()) == 40 and int((L == 1).sum()) == 60
    for n in (2, 64, 65, 128):
        assert int((L == n).sum()) >= 1
    assert int(torch.bincount(R.mixed(512)["seg"]).max()) == 1000 and R.mixed(16, scal=False)["scal"] is None
    L = torch.bincount(R.relations(16)["seg"], minlength=5)
    assert int((L == 0).sum()) == 1 and int(L.sum()) == 20000
    L = torch.bincount(R.many_hubs(16)["seg"], minlength=5000)
    assert int(L.min()) >= 65 and int(L.max()) <= 70 and L.numel() > 4096
    lt = R.loop_t(16)
    assert int((torch.bincount(lt["seg"], minlength=lt["nseg"]) > 0).sum()) == 1
    assert R.empty(16)["seg"].numel() == 0 and R.empty(16)["nseg"] == 17


@pytest.mark.parametrize("D", [1, 7, 16, 100, 200])
@pytest.mark.parametrize("mode", R.MODES)
def test_float32_emulation_stays_inside_the_bound(mode, D):
    from mr_gnas_amd import graph
    assert graph.CHUNK_EDGES == R.CHUNK
    c = R.mixed(D, nseg=40, hub=150, n_empty=5, n_one=10)
    plan = graph.dst_csr_plan_torch(c["seg"], c["nseg"])
    assert plan["n_hubs"] >= 3                                     # the hub, 65 and 128: split lists are emulated too
    ref, A, L = R.gcs_ref(mode, c["X"], c["xi"], c["Y"], c["yi"], c["scal"], c["seg"], c["nseg"])
    tol = R.gcs_bound(mode, D, A, L)
    got = R.emulate32(mode, c, plan)
    used, _, _, zero_err = R.used_fraction(got, ref, tol)
    print(f"{mode} D={D}: float32 emulation uses {used:.3f} of the bound")
    assert zero_err == 0.0 and bool((got[L == 0] == 0).all())
    assert used <= 1.0
    assert bool((tol[L > 0] > 0).all())
    if mode in R.CORR_MODES:
        # the bound can fail: without the last product, most elements of the one-element lists are outside it
        bad = R.emulate32(mode, c, plan, drop_last=True)
        ones = L == 1
        out = (bad.double() - ref).abs()[ones] > tol[ones]
        assert float(out.double().mean()) >= 0.5, float(out.double().mean())
