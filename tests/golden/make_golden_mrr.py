#!/usr/bin/env python3
"""Generate mrr_small.npz / mrr_odd.npz by RUNNING THE REFERENCE's link-prediction evaluation, utils/utils_rgcn.py:212-380
(perturb_and_get_raw_rank, perturb_s_/perturb_o_and_get_filtered_rank, calc_raw_mrr, calc_mrr), through the stand-ins of
make_golden.py (which stays as it is; see its docstring for what the stand-ins supply and where to run this).

    python tests/golden/make_golden_mrr.py

Cases
  small   N = 161 entities (one 128-column block plus 33), D = 52 (the smallest reduction length of the split-bf16 core), R = 3
  odd     N = 333, D = 50 (the exact-f32 core)
each with 400 train, 40 valid and 60 test triples, among the test triples: a duplicate (1 = 0), one also in train (2), one also in
valid (3), two sharing (r, o) (4, 5) and two sharing (s, r) (6, 7).

Stored: the embeddings (standard normal x 0.4) and relation weights, the three triple sets, the reference's 0-based ranks + 1 of both
passes (ranks_s, ranks_o) under both protocols, and mrr / hits@1,3,10: filtered from the reference's calc_mrr, raw mrr from
calc_raw_mrr (the reference's calc_mrr(eval_p="raw") fails at unpacking calc_raw_mrr's single return value) with the hits formed
from the raw ranks by the reference's formula.

The filtered ranks follow the reference's use of ONE filter set for both passes, pass S first: filter_s / filter_o remove the query's
own triple from the set for good.

Seed search.  The reference's torch.sort leaves equal scores in unspecified order, and a float32 device kernel may order two scores
that differ by rounding differently.  The generator therefore walks seeds and keeps the first where, in float64, every query's
target is separated from EVERY other candidate by more than
    delta_q = 3 * D * 2^-24 * max_e sum_c |q_c * emb[e, c]|,      q = emb[a] * w[r]
-- the float32 chain bound of two sums of D products, times the 1.5 x that include/mrgnas.h pins the split core to.  With that margin
exact rank equality may be demanded of every query; the generator asserts that the reference's ranks equal the float64 ranks and
prints the seed.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, _install_standins  # noqa: E402

CASES = {"small": dict(N=161, D=52, R=3), "odd": dict(N=333, D=50, R=3)}
N_TRAIN, N_VALID, N_TEST = 400, 40, 60


def draw(case, seed):
    N, D, R = case["N"], case["D"], case["R"]
    rng = np.random.default_rng(seed)
    tri = lambda n: np.stack([rng.integers(0, N, n), rng.integers(0, R, n), rng.integers(0, N, n)], 1).astype(np.int64)
    train, valid, test = tri(N_TRAIN), tri(N_VALID), tri(N_TEST)
    test[1] = test[0]                                             # a duplicate test triple
    test[2] = train[0]                                            # also in train
    test[3] = valid[0]                                            # also in valid
    test[5] = [(test[4, 0] + 1) % N, test[4, 1], test[4, 2]]      # shares (r, o)
    test[7] = [test[6, 0], test[6, 1], (test[6, 2] + 1) % N]      # shares (s, r)
    emb = (rng.standard_normal((N, D)) * 0.4).astype(np.float32)
    w = rng.standard_normal((R, D)).astype(np.float32)
    return emb, w, train, valid, test


def separated(emb, w, test):
    """Every query's target further than delta_q from every other candidate, in float64."""
    e64, w64 = emb.astype(np.float64), w.astype(np.float64)
    D = emb.shape[1]
    for fixed, tgt in ((test[:, 2], test[:, 0]), (test[:, 0], test[:, 2])):
        q = e64[fixed] * w64[test[:, 1]]
        x = q @ e64.T
        delta = 3 * D * 2.0 ** -24 * (np.abs(q) @ np.abs(e64).T).max(axis=1)
        gap = np.abs(x - x[np.arange(len(tgt)), tgt][:, None])
        gap[np.arange(len(tgt)), tgt] = np.inf
        if not (gap.min(axis=1) > delta).all():
            return False
    return True


def ranks64(emb, w, fixed, rel, tgt, allowed):
    """1-based float64 ranks over the candidates allowed[i] (bool [N], target included)."""
    e64 = emb.astype(np.float64)
    x = (e64[fixed] * w.astype(np.float64)[rel]) @ e64.T
    out = []
    for i in range(len(tgt)):
        out.append(1 + int(((x[i] > x[i, tgt[i]]) & allowed[i]).sum()))
    return np.array(out, dtype=np.int64)


def run_case(ur, name, case):
    for seed in range(1000):
        emb, w, train, valid, test = draw(case, seed)
        if separated(emb, w, test):
            break
    else:
        raise SystemExit(f"{name}: no separated seed")
    N, T = case["N"], len(test)
    E, W = torch.from_numpy(emb), torch.from_numpy(w)
    tr, va, te = (torch.from_numpy(t) for t in (train, valid, test))
    s, r, o = te[:, 0], te[:, 1], te[:, 2]
    with torch.no_grad():
        raw_s = ur.perturb_and_get_raw_rank(E, W, o, r, s, T, 100) + 1
        raw_o = ur.perturb_and_get_raw_rank(E, W, s, r, o, T, 100) + 1
        known = {tuple(t) for t in torch.cat([tr, va, te]).tolist()}       # calc_filtered_mrr's set: shared by both passes, S first
        fil_s = ur.perturb_s_and_get_filtered_rank(E, W, s, r, o, T, known) + 1
        fil_o = ur.perturb_o_and_get_filtered_rank(E, W, s, r, o, T, known) + 1
    mrr_f, hits_f = ur.calc_mrr(E, W, tr, va, te, hits=[1, 3, 10], eval_bz=100, eval_p="filtered")
    mrr_r = ur.calc_raw_mrr(E, W, te, hits=[1, 3, 10], eval_bz=100)
    raw = torch.cat([raw_s, raw_o])
    hits_r = [torch.mean((raw <= k).float()).item() for k in (1, 3, 10)]
    assert abs(torch.mean(1.0 / raw.float()).item() - mrr_r) == 0 and abs(torch.mean(1.0 / torch.cat([fil_s, fil_o]).float()).item() - mrr_f) == 0

    # the float64 restatement with the reference's removal order must give the same ranks (that is what the margin is for)
    full = {tuple(t) for t in np.concatenate([train, valid, test]).tolist()}
    everything = np.ones((T, N), dtype=bool)
    assert (ranks64(emb, w, test[:, 2], test[:, 1], test[:, 0], everything) == raw_s.numpy()).all()
    assert (ranks64(emb, w, test[:, 0], test[:, 1], test[:, 2], everything) == raw_o.numpy()).all()
    live = set(full)
    al_s = np.ones((T, N), dtype=bool)
    for i, (a, b, c) in enumerate(test.tolist()):
        live.discard((a, b, c))
        al_s[i] = [(e, b, c) not in live for e in range(N)]
    al_o = np.ones((T, N), dtype=bool)
    for i, (a, b, c) in enumerate(test.tolist()):
        al_o[i] = [(a, b, e) not in live for e in range(N)]
    assert (ranks64(emb, w, test[:, 2], test[:, 1], test[:, 0], al_s) == fil_s.numpy()).all()
    assert (ranks64(emb, w, test[:, 0], test[:, 1], test[:, 2], al_o) == fil_o.numpy()).all()

    np.savez_compressed(os.path.join(OUT, f"mrr_{name}.npz"), emb=emb, w=w, train=train, valid=valid, test=test, seed=np.int64(seed),
                        raw_ranks_s=raw_s.numpy(), raw_ranks_o=raw_o.numpy(), filtered_ranks_s=fil_s.numpy(), filtered_ranks_o=fil_o.numpy(),
                        raw_mrr=np.float64(mrr_r), raw_hits=np.array(hits_r, dtype=np.float64),
                        filtered_mrr=np.float64(mrr_f), filtered_hits=np.array(hits_f, dtype=np.float64))
    print(f"mrr_{name}: seed {seed}, N {N} D {case['D']} T {T}, raw mrr {mrr_r:.6f} filtered mrr {mrr_f:.6f}")


def main():
    _install_standins()
    import utils.utils_rgcn as ur
    for name, case in CASES.items():
        run_case(ur, name, case)


if __name__ == "__main__":
    main()
