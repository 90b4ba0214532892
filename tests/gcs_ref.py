"""Float64 reference, a-priori error bound and case generators for the fused gather -> compose -> segmented sum
(csrc/fused_gcs.hip: mrg_fused_gcs in its six modes, mrg_span_gcs in its four).  Plain helper module, imported by
tests/test_gcs_cpu.py (which checks this checker on the CPU) and tests/test_gcs_gpu.py.

The bound (gcs_bound) is the textbook forward error bound of a sum of float32 products in ANY association; it is derived
from the operation counts and the unit roundoff, never from what a kernel returns.  It is loose on hub rows and sharp on
short lists, so every width is run on the `mixed` case, which carries segments of length 0, 1 and 2."""
import torch

MODES = ("sub", "mul", "copy", "negs", "ccorr", "cconv")
SPAN_MODES = ("sub", "mul", "copy", "negs")
CORR_MODES = ("ccorr", "cconv")
UNIT = 2.0 ** -24                    # unit roundoff of float32
CHUNK = 64                           # graph.CHUNK_EDGES: the `mixed` case puts lists at 64, 65 and 128 elements


# ---- circular correlation / convolution ----------------------------------------------------------------------------------------
def corr64(a, b):
    """corr(a, b)[k] = sum_i a[i] b[(i + k) % D] as irfft(conj(rfft(a)) * rfft(b), n=D) over the last axis, in the
    operands' own dtype and device (float64 on the host in every reference of the tests)."""
    D = a.shape[-1]
    if a.numel() == 0 or b.numel() == 0:                    # (the host FFT refuses an empty batch)
        return a * b
    return torch.fft.irfft(torch.conj(torch.fft.rfft(a, dim=-1)) * torch.fft.rfft(b, dim=-1), n=D, dim=-1)


def conv64(a, b):
    """conv(a, b)[k] = sum_i a[i] b[(k - i) % D] as irfft(rfft(a) * rfft(b), n=D)."""
    D = a.shape[-1]
    if a.numel() == 0 or b.numel() == 0:
        return a * b
    return torch.fft.irfft(torch.fft.rfft(a, dim=-1) * torch.fft.rfft(b, dim=-1), n=D, dim=-1)


def direct64(a, b, conv=False):
    """The double sum itself (O(D^2) values per row: small D only)."""
    D = a.shape[-1]
    k, i = torch.arange(D, device=a.device)[:, None], torch.arange(D, device=a.device)[None, :]
    idx = (k - i) % D if conv else (i + k) % D              # idx[k, i]
    return (a.unsqueeze(-2) * b[..., idx]).sum(-1)


# ---- the six modes (include/mrgnas.h, MRG_GCS_*) -----------------------------------------------------------------------------------
def message(mode, x, y, s):
    """Per-element message in the operands' dtype; s is [E, 1] (ones when the kernel gets no scale)."""
    if mode == "sub":
        return x - y * s
    if mode == "mul":
        return x * (y * s)
    if mode == "copy":
        return x * s
    if mode == "negs":
        return -(x * s)
    if mode == "ccorr":
        return corr64(x, y * s)
    if mode == "cconv":
        return s * conv64(x, y)
    raise ValueError(mode)


def message_abs(mode, x, y, s):
    """The same computation on absolute values: the sum of the magnitudes of every term of the message."""
    x, s = x.abs(), s.abs()
    if mode in ("copy", "negs"):
        return x * s
    y = y.abs()
    if mode == "sub":
        return x + y * s
    if mode == "mul":
        return x * (y * s)
    D = x.shape[-1]
    if D <= 8:
        return direct64(x, y * s, conv=(mode == "cconv"))
    return (corr64 if mode == "ccorr" else conv64)(x, y * s).abs()


def gcs_ref(mode, X, xi, Y, yi, scal, seg, nseg, block=1 << 14):
    """out[v] = sum over e with seg[e] == v of message(mode, X[xi[e]], Y[yi[e]], scal[e]) in float64 on the host: the
    float32 inputs are upcast (no input rounding).  Returns (ref, A, L): A the same sums over absolute values, L[v] the
    length of segment v."""
    xi, seg = xi.long().cpu(), seg.long().cpu()
    X64 = X.detach().cpu().double()
    needs_y = mode not in ("copy", "negs")
    Y64 = Y.detach().cpu().double() if needs_y else None
    yi = yi.long().cpu() if needs_y else None
    E, D = int(seg.numel()), X64.shape[1]
    s64 = torch.ones(E, 1, dtype=torch.float64) if scal is None else scal.detach().cpu().double().view(E, 1)
    ref = torch.zeros(nseg, D, dtype=torch.float64)
    A = torch.zeros(nseg, D, dtype=torch.float64)
    for lo in range(0, E, block):
        sl = slice(lo, lo + block)
        x, y, s = X64[xi[sl]], (Y64[yi[sl]] if needs_y else None), s64[sl]
        ref.index_add_(0, seg[sl], message(mode, x, y, s))
        A.index_add_(0, seg[sl], message_abs(mode, x, y, s))
    return ref, A, torch.bincount(seg, minlength=nseg)


def gcs_bound(mode, D, A, L):
    """tol[v, k] = 1.01 * n_v * 2^-24 * A[v, k], n_v = (D if mode in (ccorr, cconv) else 2) + L[v] + 4: the
    gamma_n * sum |t_i| bound of a float32 sum of products (D - 1 adds and D products of a row, one product with the
    scale, L - 1 adds over the list in whatever chunk / hub association; 1.01 covers gamma_n = n u / (1 - n u) and the
    float64 reference's own error).  An empty segment has A = 0: its row must be exactly zero."""
    n = (D if mode in CORR_MODES else 2) + L.double() + 4
    return 1.01 * n.view(-1, 1) * UNIT * A


def used_fraction(got, ref, tol):
    """(worst err / tol over the elements with tol > 0, the err and tol at that element, the largest |err| where tol == 0)."""
    err = (got.detach().cpu().double() - ref).abs()
    if err.numel() == 0:
        return 0.0, 0.0, 0.0, 0.0
    pos = tol > 0
    ratio = torch.where(pos, err / torch.where(pos, tol, torch.ones_like(tol)), torch.zeros_like(err))
    i = int(ratio.argmax())
    zero_err = float(err[~pos].max()) if bool((~pos).any()) else 0.0
    return float(ratio.view(-1)[i]), float(err.view(-1)[i]), float(tol.view(-1)[i]), zero_err


# ---- cases ------------------------------------------------------------------------------------------------------------------------
def _finish(gen, D, lens, n_x, n_y, scal, shuffle=True):
    lens = torch.as_tensor(lens, dtype=torch.long)
    nseg = int(lens.numel())
    seg = torch.repeat_interleave(torch.arange(nseg), lens)
    E = int(seg.numel())
    if shuffle and E:
        seg = seg[torch.randperm(E, generator=gen)]
    return dict(D=D, nseg=nseg, seg=seg, n_x=n_x, n_y=n_y,
                X=torch.randn(n_x, D, generator=gen), Y=torch.randn(n_y, D, generator=gen),
                xi=torch.randint(0, n_x, (E,), generator=gen), yi=torch.randint(0, n_y, (E,), generator=gen),
                scal=(torch.rand(E, generator=gen).clamp_(min=1e-3) if scal else None))


def mixed(D, scal=True, seed=11, nseg=300, hub=None, n_empty=40, n_one=60):
    """One hub, empty segments, segments of one element, one each at 64, 65 and 128 elements (the chunk boundary), the
    rest 2..12 (at least one of exactly 2); segment ids and edge order shuffled."""
    gen = torch.Generator().manual_seed(seed + 1000 * D)
    hub = (1000 if D >= 512 else 9000) if hub is None else hub
    rest = nseg - 1 - n_empty - n_one - 3
    assert rest >= 1
    small = torch.randint(2, 13, (rest,), generator=gen)
    small[0] = 2
    lens = torch.cat((torch.tensor([hub]), torch.zeros(n_empty, dtype=torch.long), torch.ones(n_one, dtype=torch.long),
                      torch.tensor([CHUNK, CHUNK + 1, 2 * CHUNK]), small))
    lens = lens[torch.randperm(nseg, generator=gen)]
    return _finish(gen, D, lens, 500, 11, scal)


def relations(D, seed=12):
    """The shape of a relation-keyed backward plan: five segments, one of them empty, every other one a long hub."""
    gen = torch.Generator().manual_seed(seed + 1000 * D)
    return _finish(gen, D, [7000, 0, 4000, 8000, 1000], 500, 11, True)


def loop(D, seed=13, N=3000, n_y=11):
    """The self-loop plan of compgcn._layer_plans: element v reads node row v and ONE constant relation row, segment v."""
    gen = torch.Generator().manual_seed(seed + 1000 * D)
    c = _finish(gen, D, torch.ones(N, dtype=torch.long), N, n_y, False, shuffle=False)
    c["xi"] = torch.arange(N)
    c["yi"] = torch.full((N,), n_y - 1, dtype=torch.long)
    return c


def loop_t(D, seed=14, N=3000, n_y=11):
    """The transpose of `loop`, keyed by the relation row (its d/dr plan): one segment holds all N elements, the other
    n_y - 1 are empty; both operands are read row by row."""
    gen = torch.Generator().manual_seed(seed + 1000 * D)
    lens = torch.zeros(n_y, dtype=torch.long)
    lens[n_y - 1] = N
    c = _finish(gen, D, lens, N, N, False, shuffle=False)
    c["xi"] = torch.arange(N)
    c["yi"] = torch.arange(N)
    return c


def many_hubs(D, seed=15, nseg=5000):
    """More split lists than the hub kernel's grid (4096 workgroups): every segment has 65..70 elements."""
    gen = torch.Generator().manual_seed(seed + 1000 * D)
    return _finish(gen, D, torch.randint(65, 71, (nseg,), generator=gen), 500, 11, True)


def empty(D, seed=16, nseg=17):
    gen = torch.Generator().manual_seed(seed + 1000 * D)
    return _finish(gen, D, torch.zeros(nseg, dtype=torch.long), 500, 11, True)


# ---- float32 emulation of the kernels' summation (plain torch, CPU) --------------------------------------------------------------
def emulate32(mode, c, plan, drop_last=False):
    """The chunk kernels' arithmetic in float32 with torch on the host: products over i ascending, times the scale,
    each chunk of the plan (graph.dst_csr_plan_torch) summed in list order, a split list's partials added in order.
    drop_last leaves out the product at i = D - 1 of the two O(D^2) modes (a kernel that loses its last window step)."""
    D, nseg = c["D"], c["nseg"]
    E = int(c["seg"].numel())
    x = c["X"][c["xi"]]
    y = c["Y"][c["yi"]]
    s = c["scal"].view(E, 1) if c["scal"] is not None else torch.ones(E, 1)
    if mode in CORR_MODES:
        k = torch.arange(D)
        p = torch.zeros(E, D)
        for i in range(D - 1 if drop_last else D):
            p = p + x[:, i:i + 1] * y[:, (i + k) % D if mode == "ccorr" else (k - i) % D]
        msg = p * s
    else:
        msg = message(mode, x, y, s)
    assert msg.dtype == torch.float32
    out = torch.zeros(nseg, D)
    part = {}
    eid = plan["eid"].long()
    for ch in range(plan["n_chunks"]):
        v, j0, j1, slot = (int(plan[k_][ch]) for k_ in ("chunk_node", "chunk_start", "chunk_end", "chunk_slot"))
        acc = torch.zeros(D)
        for j in range(j0, j1):
            acc = acc + msg[eid[j]]
        if slot < 0:
            out[v] = acc
        else:
            part[slot] = acc
    for h in range(plan["n_hubs"]):
        v, s0, cnt = (int(plan[k_][h]) for k_ in ("hub_node", "hub_first", "hub_count"))
        acc = torch.zeros(D)
        for q in range(s0, s0 + cnt):
            acc = acc + part[q]
        out[v] = acc
    return out
