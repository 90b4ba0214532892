"""The seeded inputs and the output set of the register-tiled [queries, entities] sweeps' bit fixture (tests/golden/sweep_1n_bits.npz),
shared by tools/lab/record_sweep_bits.py (which recorded it ONCE, from the build with one kernel file per scorer count) and
tests/test_sweep_bits_gpu.py (which demands the same bits of every later build).  Inputs are generated, never stored.

Everything is drawn on the CPU from seeded generators.  The operands are scaled as test_sf_mix3_gpu.mix3_case scales them -- distances
spanning at most 13 with gamma in their middle, |(sub * rel) . ent| <= 7, |hidden . ent| <= 7: no probability saturates -- but every
scale is rounded DOWN TO A POWER OF TWO and gamma to a multiple of 1/64: a float64 sum that lands an ulp elsewhere on another host
cannot move an input bit.  `hot` multiplies operands and gamma by 20: most probabilities are 0 or 1 in float32.

Shapes (B, N, D), the smallest that reach every edge of the 64 x 64 x 32 tile:
  (65, 130, 40)          float4 staging, two row tiles, a ragged third column tile, two LDS slices
  (129, 193, 33)         scalar staging, a ragged last slice
  (63, 64, 1)            a single column (N = 64: there is no column range (64, N))
  (2, 28672 + 65, 36)    a second column block: partials appended across launches
Arrays of more than FULL elements are kept as the SHA-256 of their bytes (and their float64 sum, for the eye); the rest in full.
FULL is 2 048, not 65 536: the gradient slices of the three small shapes are 4 032 to 24 897 floats each, about 150 of them, and kept
in full they alone would be megabytes.  A digest pins the same bits."""
import hashlib

import numpy as np
import torch

from mr_gnas_amd import evaluation as EV, functional as K
from mr_gnas_amd.sampler import LabelIndex

DEV = "cuda"
R = 3
LABEL_SMOOTH = 0.1
TOPK = 10
FULL = 2048
INT32_MAX = 2 ** 31 - 1
# name -> (B, N, D, hot)
CASES = {"b65_n130_d40": (65, 130, 40, False), "b129_n193_d33": (129, 193, 33, False), "b63_n64_d1": (63, 64, 1, False),
         "b2_n28737_d36": (2, 28672 + 65, 36, False), "b65_n130_d40_hot": (65, 130, 40, True), "b129_n193_d33_hot": (129, 193, 33, True)}
WEIGHTS = {2: {"mix": (0.3, 0.7), "hot0": (1.0, 0.0), "hot1": (0.0, 1.0)},
           3: {"mix": (0.4, 0.35, 0.25), "hot0": (1.0, 0.0, 0.0), "hot2": (0.0, 0.0, 1.0)}}


class Side:
    """A filter index as plain tensors, in the layout evaluation.query_ranks reads."""

    def __init__(self, keys, rowptr, members, gone_at):
        self.keys, self.num_rels = keys.long().to(DEV), R
        self.rowptr, self.members, self.gone_at = (t.int().contiguous().to(DEV) for t in (rowptr, members, gone_at))


def _pow2_floor(x):
    return 2.0 ** int(np.floor(np.log2(x)))


def _dist64(obj, ent):
    obj, ent = obj.double(), ent.double()
    return torch.cat([(obj[i:i + 16].unsqueeze(1) - ent.unsqueeze(0)).abs().sum(-1) for i in range(0, obj.shape[0], 16)])


def make_inputs(name):
    """{ent, sub, rel, hidden, gamma, li, subj, relid, qkey_l, side, when, qkey_r, t} of a case: the float operands on the device, the
    label index of the losses (key (0, 0) lists every entity, key (1, 0) entities 63 and 64) and the filter index of the ranks (gone_at
    below, at and above `when`; query 1 has everything filtered, query 2 an unknown key)."""
    B, N, D, hot = CASES[name]
    seed = 1000003 * B + 1009 * N + D
    gen = torch.Generator().manual_seed(seed)
    ent, sub, rel = (torch.randn(n, D, generator=gen) for n in (N, B, B))
    hidden = torch.relu(torch.randn(B, D, generator=gen))
    d = _dist64(sub + rel, ent)
    f = _pow2_floor(min(1.0, 13.0 / max(float(d.max() - d.min()), 1e-30)))
    x1 = ((f * sub).double() * (f * rel).double()) @ (f * ent).double().T
    f *= _pow2_floor(min(1.0, (7.0 / max(float(x1.abs().max()), 1e-30)) ** (1.0 / 3.0)))
    ent, sub, rel = f * ent, f * sub, f * rel
    d = _dist64(sub + rel, ent)
    gamma = round(0.5 * float(d.max() + d.min()) * 64.0) / 64.0
    hidden = _pow2_floor(min(1.0, 7.0 / max(float((hidden.double() @ ent.double().T).abs().max()), 1e-30))) * hidden
    assert float((gamma - d).abs().max()) <= 7.0 and float(((sub * rel).double() @ ent.double().T).abs().max()) <= 7.0
    if hot:
        ent, sub, rel, hidden, gamma = 20.0 * ent, 20.0 * sub, 20.0 * rel, 20.0 * hidden, 20.0 * gamma

    rng = np.random.default_rng(seed)
    T = 3 * N
    tri = np.stack([rng.integers(0, N, T), rng.integers(0, R - 1, T), rng.integers(0, N, T)], 1)
    extra = [(0, 0, o) for o in range(N)] + [(min(1, N - 1), 0, o) for o in (63, 64) if o < N]
    tri = np.concatenate([tri, np.asarray(extra, dtype=tri.dtype)])
    subj, relid = rng.integers(0, N, B), rng.integers(0, 2 * R, B)
    for i, (s, r) in enumerate([(0, 0), (min(1, N - 1), 0), (int(rng.integers(0, N)), R - 1)][:B]):
        subj[i], relid[i] = s, r
    li = LabelIndex(tri, R, N, DEV)
    subj, relid = torch.from_numpy(subj).to(DEV), torch.from_numpy(relid).to(DEV)

    ri = lambda lo, hi, n: torch.randint(lo, hi, (n,), generator=gen)
    t, when, qkey_r = ri(0, N, B), ri(-1, 10, B), torch.arange(B) % 9
    t[0], t[B - 1] = 0, N - 1
    edges = torch.tensor([c for c in (0, 63, 64, 127, 128, N - 1) if c < N])
    lists = [(torch.arange(N), torch.full((N,), INT32_MAX))]                  # key 0: every entity, for good
    for k in range(1, 9):
        m = torch.unique(torch.cat((edges, ri(0, N, N // (2 + k % 3) + 1)))) if k != 5 else torch.empty(0, dtype=torch.int64)
        lists.append((m, ri(0, 10, m.numel())))
    qkey_r[0], qkey_r[1 % B] = 3, 0
    if B > 2:
        qkey_r[2] = -1
    rowptr = torch.tensor([0] + [m.numel() for m, _ in lists]).cumsum(0)
    side = Side(torch.arange(9), rowptr, torch.cat([m for m, _ in lists]), torch.cat([g for _, g in lists]))
    return dict(ent=ent.to(DEV), sub=sub.to(DEV), rel=rel.to(DEV), hidden=hidden.to(DEV), gamma=float(gamma), li=li, subj=subj, relid=relid,
                qkey_l=(subj.long() * (2 * R) + relid.long()).contiguous(), side=side, when=when.int().to(DEV), qkey_r=qkey_r.to(DEV),
                t=t.int().to(DEV))


def _w(w):
    return torch.tensor(w, dtype=torch.float32, device=DEV)


def _all_grads(fn, leaves):
    leaves = [x.detach().clone().requires_grad_(True) for x in leaves]
    loss = fn(*leaves)
    (3.0 * loss).backward()
    return [loss.detach()] + [x.grad for x in leaves]


def outputs(name):
    """{key: CPU tensor} of everything the fixture pins for a case, from the library that is loaded."""
    c = make_inputs(name)
    B, N, D, _ = CASES[name]
    ent, sub, rel, hidden, gamma, li, qkey = c["ent"], c["sub"], c["rel"], c["hidden"], c["gamma"], c["li"], c["qkey_l"]
    obj, qd = (sub + rel).contiguous(), (sub * rel).contiguous()
    v0, v1 = li.label_values(LABEL_SMOOTH)
    gscale = torch.full((1,), 3.0 / (B * N), device=DEV)
    ranges = [(0, N)] + ([(64, N)] if N > 64 else [])
    filt = (c["side"], c["when"], c["qkey_r"])
    out = {}
    with torch.no_grad():
        out["l1/loss"] = K.transe_bce_mean(obj, ent, gamma, li, qkey, v0, v1)
        for c0, c1 in ranges:
            out[f"l1/dl_{c0}"] = K.transe_bce_dlogit(obj, ent, gamma, li, qkey, v0, v1, c0, c1, gscale)
        out["l1/rank"] = EV.query_ranks(obj, ent, c["t"], *filt, kind="l1")
        out["l1/rank_raw"] = EV.query_ranks(obj, ent, c["t"], kind="l1")
        out["l1/topk_ids"], out["l1/topk_vals"] = EV.query_topk(obj, ent, min(TOPK, N), *filt, kind="l1")
        out["l1/topk_raw_ids"], out["l1/topk_raw_vals"] = EV.query_topk(obj, ent, min(TOPK, N), kind="l1")
        for ns in (2, 3):
            dots, hid = ((qd,), {}) if ns == 2 else ((qd, hidden), {"hidden": hidden})
            mean, grad = (K.sf_mix_bce_mean, K.sf_mix_bce_grad) if ns == 2 else (K.sf_mix3_bce_mean, K.sf_mix3_bce_grad)
            for wn, w in WEIGHTS[ns].items():
                p, ww = f"mix{ns}/{wn}/", _w(w)
                out[p + "loss"] = mean(obj, *dots, ent, ww, gamma, li, qkey, v0, v1)
                for c0, c1 in ranges:
                    *dl, dw = grad(obj, *dots, ent, ww, gamma, li, qkey, v0, v1, c0, c1, gscale, dw=torch.full((ns,), 0.25, device=DEV))
                    out.update({f"{p}dl{k}_{c0}": x for k, x in enumerate(dl)})
                    out[f"{p}dw_{c0}"] = dw
                out[p + "rank"] = EV.mix_ranks(sub, rel, ent, ww, gamma, c["t"], *filt, **hid)
                out[p + "rank_raw"] = EV.mix_ranks(sub, rel, ent, ww, gamma, c["t"], **hid)
    for ns, names in ((2, ("ent", "sub", "rel", "w")), (3, ("ent", "sub", "rel", "hidden", "w"))):
        if ns == 2:
            fn = lambda e, s, r, w: K.sf_mix_bce_all(e, s, r, w, gamma, li, c["subj"], c["relid"], LABEL_SMOOTH, 64)
            leaves = (ent, sub, rel, _w(WEIGHTS[2]["mix"]))
        else:
            fn = lambda e, s, r, h, w: K.sf_mix3_bce_all(e, s, r, h, w, gamma, li, c["subj"], c["relid"], LABEL_SMOOTH, 64)
            leaves = (ent, sub, rel, hidden, _w(WEIGHTS[3]["mix"]))
        res = _all_grads(fn, leaves)
        out.update({f"mix{ns}/all/{k}": x for k, x in zip(("loss",) + tuple("g_" + n for n in names), res)})
    torch.cuda.synchronize()
    return {k: v.detach().cpu() for k, v in out.items()}


def pack(tensors):
    """{key: numpy array} as the fixture stores a case's outputs: arrays of at most FULL elements as they are; of the others the
    names ('#names'), the SHA-256 of their bytes ('#sha' [n, 32]) and their float64 sums ('#sum' [n])."""
    res, names, sha, sums = {}, [], [], []
    for k, v in tensors.items():
        a = np.ascontiguousarray(v.numpy())
        if a.size > FULL:
            names.append(k)
            sha.append(np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8))
            sums.append(float(a.sum(dtype=np.float64)))
        else:
            res[k] = a
    res["#names"], res["#sha"], res["#sum"] = np.array(names), np.stack(sha), np.array(sums, dtype=np.float64)
    return res
