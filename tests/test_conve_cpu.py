"""ConvE scorers on the host side: CompGCN_ConvE exists with the reference's constructor and parameter names
(models/compgcn.py:188-269), and sf_ConvE_op on CPU tensors still runs torch's formulation and matches the reference's fixture
(models/operations_lp.py:150-205)."""
import inspect

import torch

from conftest import load_golden, sub


def test_compgcn_conve_signature_and_state_dict_match_the_reference():
    from mr_gnas_amd.compgcn import CompGCN_ConvE
    z = load_golden("conve_compgcn_small")
    assert str(inspect.signature(CompGCN_ConvE.__init__)) == z["signature"]
    net = CompGCN_ConvE(z["nb"], 2 * z["R"], z["N"], z["Din"], [z["Dout"]], comp_fn="sub", dropout=0.0, layer_dropout=[0.0],
                        num_filt=z["F"], hid_drop=0.0, feat_drop=0.0, ker_sz=z["ks"], k_w=z["k_w"], k_h=z["k_h"])
    ours = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    ref = {k: tuple(v.shape) for k, v in sub(z, "param0/").items()}
    assert ours == ref
    assert sorted(n for n, _ in net.named_parameters()) == sorted(sub(z, "pshape/"))


def test_compgcn_conve_refuses_a_mis_shaped_image():
    import pytest
    from mr_gnas_amd.compgcn import CompGCN_ConvE
    net = CompGCN_ConvE(0, 4, 10, 8, [20], ker_sz=3, k_w=5, k_h=5)
    with pytest.raises(ValueError, match="k_w \\* k_h"):
        net(None, torch.zeros(2, dtype=torch.long), torch.zeros(2, dtype=torch.long))


def sf_case(z, tag):
    from mr_gnas_amd import operations_lp as O
    B, N, D, k_h, k_w, ks, F = (int(v) for v in z[f"{tag}/args"])
    op = O.sf_ConvE_op({"embed_dim": D, "conve_hid_drop": 0.0, "feat_drop": 0.0, "num_filt": F, "ker_sz": ks, "k_w": k_w, "k_h": k_h})
    op.load_state_dict(sub(z, f"{tag}/param0/"))
    return op


def test_sf_conve_cpu_path_is_unchanged():
    z = load_golden("conve_sf_small")
    for tag in ("s0", "s1", "s2"):
        op = sf_case(z, tag)
        ins = [z[f"{tag}/{n}"].clone().requires_grad_(True) for n in ("ent", "sub", "rel")]
        op.train()
        pred = op(*ins)
        loss = torch.nn.functional.binary_cross_entropy(pred, z[f"{tag}/label"])
        loss.backward()
        torch.testing.assert_close(pred, z[f"{tag}/pred"], rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(loss.detach(), z[f"{tag}/loss"], rtol=1e-5, atol=1e-7)
        for t, n in zip(ins, ("gent", "gsub", "grel")):
            torch.testing.assert_close(t.grad, z[f"{tag}/{n}"], rtol=1e-4, atol=1e-6)
        for n, p in op.named_parameters():
            torch.testing.assert_close(p.grad, z[f"{tag}/gparam/{n}"], rtol=1e-4, atol=1e-6)
        bufs = dict(op.named_buffers())
        for n, ref in sub(z, f"{tag}/buffer/").items():
            torch.testing.assert_close(bufs[n], ref, rtol=1e-5, atol=1e-6)
        op.eval()
        with torch.no_grad():
            torch.testing.assert_close(op(*ins), z[f"{tag}/pred_eval"], rtol=1e-5, atol=1e-6)
