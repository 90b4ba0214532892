"""What the row-geometry tests share (test_row_geometry_cpu.py pins it without a GPU, test_row_geometry_gpu.py runs the kernels):

  a. the width list -- the first and last width of every <VEC, LPR, KMAX> class of csrc/row_geom.hpp, aligned, scalar and forced
     scalar by a base 4 bytes past a 16-byte boundary -- and the widths every family must refuse;
  b. the row counts and direction bounds, the segment-reducer block;
  c. what the host code of mixedop.hip / cell_zero.hip admits at a width (largest K of forward and of backward);
  d. plain torch restatements of the row-streaming operators, dtype-agnostic: float64 in, float64 out, gradients by autograd;
  e. the conditioning of seeded inputs, so that float32 and float64 can differ by rounding only and never by a decision (the sign
     of a ReLU argument, the winner of a maximum)."""
import functools

import torch

from conftest import seeded

# ---- a. widths --------------------------------------------------------------------------------------------------------------------
ALIGNED = [4, 64, 68, 128, 132, 256, 260, 512, 516, 768, 772, 1024]
SCALAR = [1, 15, 17, 31, 33, 63, 65, 127, 129, 191, 193, 255]
FORCED_SCALAR = [16, 64, 128, 200, 256]                         # at a base that is not 16-byte aligned
CONFIGS = [(D, False) for D in ALIGNED + SCALAR] + [(D, True) for D in FORCED_SCALAR]
REFUSED = [(1028, False), (258, False), (260, True), (512, True)]      # what every family returns MRG_E_SHAPE for before any launch
REFUSAL_EDGES = [(1028, False), (257, False), (260, True)]              # the first refused width of each placement (the host check)
CLASSES = ["A16", "A32", "A64k1", "A64k2", "A64k4", "S16", "S32", "S64k1", "S64k2", "S64k4"]


def arg_of(D, unaligned):
    """The (width, placement) pair as tools/row_geom_check.cpp takes it."""
    return f"{D}u" if unaligned else str(D)


def geom(D, unaligned):
    """(vec, lpr, kmax, live steps) of csrc/row_geom.hpp, or None for a refused width (test_row_geometry_cpu.py holds this
    restatement against the C++ function over the whole list)."""
    vec = 4 if (D % 4 == 0 and not unaligned) else 1
    dv = D // vec
    lpr = 16 if dv <= 16 else (32 if dv <= 32 else 64)
    k = -(-dv // lpr)
    if D <= 0 or k > 4:
        return None
    return vec, lpr, (1 if k <= 1 else 2 if k <= 2 else 4), k


def class_of(D, unaligned):
    g = geom(D, unaligned)
    if g is None:
        return None
    vec, lpr, kmax, _ = g
    return ("A" if vec == 4 else "S") + str(lpr) + ("" if lpr < 64 else f"k{kmax}")


def config_id(D, unaligned):
    return f"{class_of(D, unaligned)}-D{arg_of(D, unaligned)}"


def place(t, unaligned=False, device="cuda"):
    """The tensor on the device; `unaligned`: contiguous rows whose base is 4 bytes past a 16-byte boundary."""
    if t is None:
        return None
    if not unaligned:
        return t.to(device)
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


# ---- b. rows ------------------------------------------------------------------------------------------------------------------------
# M -> (b0, b1): one row per direction segment; an empty first segment; ragged against every rows-per-block (16, 8, 4 row groups of
# a 256-thread block, times 4 or 8 rows each) and against the two rows in flight of the LPR = 64 gate kernels
BOUNDS = {3: (1, 2), 37: (0, 17), 1031: (400, 801)}
ROWS = (3, 37, 1031)
BN_ROWS = (37, 1031)                                             # BatchNorm in training mode needs two rows


def reducer_block(seed):
    """(src, dst, n_src, n_dst) of a block of 60 destinations: a hub of 700 in-edges (longer than one chunk of the plan), 8
    destinations without in-edges (1..8), 12 of in-degree 1 (9..20), the rest 2..9; the edge list shuffled."""
    gen = torch.Generator().manual_seed(seed)
    n_dst, n_src = 60, 90
    deg = torch.randint(2, 10, (n_dst,), generator=gen)
    deg[0], deg[1:9], deg[9:21] = 700, 0, 1
    dst = torch.repeat_interleave(torch.arange(n_dst), deg)
    dst = dst[torch.randperm(dst.numel(), generator=gen)]
    src = torch.randint(0, n_src, (int(dst.numel()),), generator=gen)
    return src, dst, n_src, n_dst


# ---- c. what the host code admits ---------------------------------------------------------------------------------------------------
MIX_MAXK = 8                                                     # MRG_MIX_MAXK (csrc/mixedop_parts.hpp)
ZERO_MAXK = 3                                                    # ZK (csrc/cell_zero.hip): the three compose kinds
LDS_FLOATS = 64 * 1024 // 4


TANH_MAXK = 5                                                    # mixedop.hip gated_pack: `gp->act == 1 && (K > 5 || ...)`, at every width


def mix_limits(D, unaligned, maxk=MIX_MAXK):
    """Largest K the MixedOp host code admits at width D: (forward, backward), 0 = not even K = 1.  The same three checks guard the
    cell-zero kernels (maxk = ZERO_MAXK); the tanh instances of the MixedOp take TANH_MAXK candidates at most (maxk = TANH_MAXK).
      forward   mrg_mix_fwd / mrg_zero_fwd:   K * 2 * D floats of LDS              (mixedop.hip `size_t lds = (size_t)K * 2 * D`, cell_zero.hip idem)
      backward  mrg_mix_bwd_reduce / mrg_zero_bwd_reduce:  K * 4 * D + (256 / LPR) * 3 * (LPR * KMAX * VEC) floats
                                              (`size_t lds = ((size_t)K * 4 * D + (size_t)(MRG_BLOCK / L) * 3 * (L * KM * V))`)
                mrg_mix_bwd_apply / mrg_zero_bwd_apply:    K * 6 * D floats         (`size_t lds = (size_t)K * 6 * D`)
    each against `lds > 64 * 1024` bytes."""
    vec, lpr, kmax, _ = geom(D, unaligned)
    fwd = min(maxk, LDS_FLOATS // (2 * D))
    red = (LDS_FLOATS - (256 // lpr) * 3 * (lpr * kmax * vec)) // (4 * D)
    return fwd, max(0, min(maxk, red, LDS_FLOATS // (6 * D)))


# ---- d. restatements ----------------------------------------------------------------------------------------------------------------
def segments(b0, b1, M):
    return ((0, b0), (b0, b1), (b1, M))


def gate_logit(s, s_in, W, b, a):
    """a(W [s ; s_in] + b) per row, [rows, 1] (reference models/operations_lp.py:317-338)."""
    x = s if s_in is None else torch.cat([s, s_in], dim=1)
    return (x @ W.t() + b) @ a.t()


def gate_row_factor(s, s_in, norm, b0, b1, params, scale=1.0 / 3.0):
    """f_sparse_comp's gate as one factor per row [M]: sigmoid(gate) * scale (* norm on the edge rows [0, b1)).  params: W, b, a of
    the in, out and self segment (None, None, None for an absent one); s_in None: a one-operand gate, W [D, D]."""
    M = s.shape[0]
    f = []
    for i, (lo, hi) in enumerate(segments(b0, b1, M)):
        W, b, a = params[3 * i:3 * i + 3]
        if W is None:
            assert hi == lo
            continue
        f.append(torch.sigmoid(gate_logit(s[lo:hi], None if s_in is None else s_in[lo:hi], W, b, a)).view(-1) * scale)
    f = torch.cat(f)
    if norm is not None:
        f = torch.cat((f[:b1] * norm.to(f.dtype).view(-1)[:b1], f[b1:]))
    return f


def gate_comp(s, s_in, norm, b0, b1, params):
    """f_sparse_comp (reference models/operations_lp.py:304-343; oracle.ops.f_sparse_comp at (b0, b1) = (E / 2, E))."""
    return s * gate_row_factor(s, s_in, norm, b0, b1, params).view(-1, 1)


def gate_last(s, W, b, a):
    """f_sparse_last (reference models/operations_lp.py:405-416; oracle.ops.f_sparse_last)."""
    return torch.sigmoid(gate_logit(s, None, W, b, a)) * s


def compose(kind, s, hr):
    return {"mult": s * hr, "sub": s - hr, "add": s + hr}[kind]


def dense_filter(kind, s, s_in, norm, b0, b1, params, self_scale):
    """kind 0: f_dense_comp, sigmoid(W [s ; s_in] + b) * s; kind 1: f_comp, W [s ; s_in]; edge rows * norm / 3, self rows * self_scale
    (reference models/operations_lp.py:356-390, 266-288; oracle.ops.f_dense_comp / f_comp).  params: W, b of the three segments."""
    M = s.shape[0]
    outs = []
    for i, (lo, hi) in enumerate(segments(b0, b1, M)):
        W, b = params[2 * i:2 * i + 2]
        x = torch.cat([s[lo:hi], s_in[lo:hi]], dim=1)
        z = x @ W.t() + (b if b is not None else 0)
        outs.append(torch.sigmoid(z) * s[lo:hi] if kind == 0 else z)
    e = torch.cat(outs[:2]) * (1.0 / 3.0) * norm.to(s.dtype).view(-1, 1)[:b1]
    return torch.cat((e, outs[2] * self_scale))


def dense_dz(kind, g, s, gate, c):
    """First backward pass of the dense filters (csrc/dense.hip): kind 0 dz = g s c gate (1 - gate), gs = g c gate; kind 1 dz = g c."""
    c = c.view(-1, 1)
    if kind == 1:
        return g * c, None
    return g * s * c * gate * (1 - gate), g * c * gate


def seg_reduce(kind, msg, self_rows, dst, n):
    """out[v] = sum | mean | max over v's in-edge rows of msg (+ self_rows[v]); 0 for a destination without in-edges."""
    D = msg.shape[1]
    if kind == "max":
        out = torch.zeros(n, D, dtype=msg.dtype).scatter_reduce(0, dst.view(-1, 1).expand(-1, D), msg, "amax", include_self=False)
    else:
        out = torch.zeros(n, D, dtype=msg.dtype).index_add(0, dst, msg)
        if kind == "mean":
            out = out / torch.bincount(dst, minlength=n).clamp(min=1).to(msg.dtype).view(-1, 1)
    return out if self_rows is None else out + self_rows


def seg_std(msg, dst, n, eps=1e-5):
    """a_std (reference models/operations.py:168-190): sqrt(relu(E[x^2] - E[x]^2) + eps) over the in-edge rows, 0 without in-edges."""
    deg = torch.bincount(dst, minlength=n).to(msg.dtype).view(-1, 1)
    d1 = deg.clamp(min=1)
    mean = torch.zeros(n, msg.shape[1], dtype=msg.dtype).index_add(0, dst, msg) / d1
    msq = torch.zeros(n, msg.shape[1], dtype=msg.dtype).index_add(0, dst, msg * msg) / d1
    return torch.where(deg > 0, torch.sqrt(torch.relu(msq - mean * mean) + eps), torch.zeros_like(mean))


def bn_arg(y, gamma, beta, training, rm, rv, eps=1e-5):
    """BatchNorm1d's output: batch statistics (biased variance) in training mode, the running ones in eval mode."""
    if training:
        mu, var = y.mean(0), y.var(0, unbiased=False)
    else:
        mu, var = rm.to(y.dtype), rv.to(y.dtype)
    return (y - mu) / torch.sqrt(var + eps) * gamma + beta


def mixed(ys, gammas, betas, w, addend=None, act="relu", training=True, rms=None, rvs=None, eps=1e-5):
    """addend + sum_k w[k] act(BatchNorm_k(ys[k])) (reference models/cell_lp.py:25-33); ys[k] None: an all-zero candidate."""
    out = 0 if addend is None else addend
    fn = torch.relu if act == "relu" else torch.tanh
    for k, y in enumerate(ys):
        ref = next(t for t in ys if t is not None)
        y = torch.zeros_like(ref) if y is None else y
        out = out + w[k] * fn(bn_arg(y, gammas[k], betas[k], training, rms[k] if rms else None, rvs[k] if rvs else None, eps))
    return out


def running_stats(y, rm, rv, momentum=0.1):
    """BatchNorm1d's running statistics after one training forward over y (unbiased variance)."""
    return (1 - momentum) * rm.to(y.dtype) + momentum * y.mean(0), (1 - momentum) * rv.to(y.dtype) + momentum * y.var(0, unbiased=True)


def cell_zero(kinds, ent, rel, ei, ri, gammas, betas, w, training=True, rms=None, rvs=None):
    """Cell zero's MixedOp over the compose candidates of the gathered rows (reference models/cell_lp.py:53-68)."""
    x, h = ent[ei], rel[ri]
    return mixed([compose(k, x, h) for k in kinds], gammas, betas, w, training=training, rms=rms, rvs=rvs)


def grads(out, gout, leaves):
    """Autograd gradients of sum(out * gout) w.r.t. the leaves that are tensors requiring grad (None for the others)."""
    idx = [i for i, t in enumerate(leaves) if t is not None and t.requires_grad]
    got = torch.autograd.grad(out, [leaves[i] for i in idx], gout.to(out.dtype), allow_unused=True)
    res = [None] * len(leaves)
    for i, g in zip(idx, got):
        res[i] = g
    return res


def f64(ts, requires_grad=True):
    """Float64 leaves of float32 tensors (None passes through)."""
    return [None if t is None else t.detach().cpu().double().requires_grad_(requires_grad) for t in ts]


def f32(ts):
    """Float32 leaves on the CPU (None passes through): the restatements evaluated as float32 torch evaluates them."""
    return [None if t is None else t.detach().cpu().float().clone().requires_grad_(True) for t in ts]


# ---- seeded inputs ------------------------------------------------------------------------------------------------------------------
def gate_params(D, in_dim, seed, present=(True, True, True)):
    """W [D, in_dim], b [D], a [1, D] per segment, xavier-sized as the reference initialises them, biases non-zero."""
    p = []
    for i, on in enumerate(present):
        if not on:
            p += [None, None, None]
            continue
        p += [seeded(f"W{i}", (D, in_dim), seed, (2.0 / (D + in_dim)) ** 0.5), seeded(f"b{i}", (D,), seed, 0.1),
              seeded(f"a{i}", (1, D), seed, (2.0 / (D + 1)) ** 0.5)]
    return p


def dense_params(D, seed, bias):
    p = []
    for i in range(3):
        p += [seeded(f"dW{i}", (D, 2 * D), seed, (2.0 / (3 * D)) ** 0.5), seeded(f"db{i}", (D,), seed, 0.1) if bias else None]
    return p


def norm_of(b1, seed):
    return (seeded("norm", (b1,), seed).abs() * 0.5 + 0.05) if b1 > 0 else torch.zeros(0)


# ---- e. conditioning ----------------------------------------------------------------------------------------------------------------
RELU_MARGIN = 1e-4            # no ReLU argument below this fraction of its column's largest magnitude
MAX_GAP = 1e-5                # the largest message of a (destination, column) leads the second largest by this fraction of the scale


def relu_margin(z):
    """Smallest |z| / column scale over a ReLU argument [rows, D] (float64)."""
    return float((z.abs() / z.abs().amax(0, keepdim=True).clamp(min=1e-300)).min())


def condition_relu(tensors, args_of, touch, seed, rounds=40):
    """Regenerates entries of the float32 `tensors` (in place) until no ReLU argument of the float64 reference is within RELU_MARGIN
    of zero.  args_of(tensors) -> list of float64 [rows, D] ReLU arguments; touch(k, bad) -> (index into tensors, boolean mask over
    that tensor) of the entries behind the offending arguments `bad` of argument k, or a list of such pairs.  Fixed seed; returns the
    margin reached."""
    gen = torch.Generator().manual_seed(seed)
    for _ in range(rounds):
        zs = args_of(tensors)
        clean = True
        for k, z in enumerate(zs):
            bad = z.abs() < 2 * RELU_MARGIN * z.abs().amax(0, keepdim=True)
            if bool(bad.any()):
                clean = False
                hits = touch(k, bad)
                for i, mask in (hits if isinstance(hits, list) else [hits]):
                    t = tensors[i]
                    t[mask] = t[mask] + (torch.randn(int(mask.sum()), generator=gen) * 0.25 * float(t.std())).to(t.dtype)
        if clean:
            break
    return min(relu_margin(z) for z in args_of(tensors))


def max_gap(msg, dst, n):
    """Smallest lead of the largest over the second largest message of a (destination, column) with two or more messages, as a
    fraction of max |msg| (float64 in)."""
    order = torch.argsort(dst, stable=True)
    m, d = msg[order], dst[order]
    deg = torch.bincount(d, minlength=n)
    worst = float("inf")
    start = 0
    for v in range(n):
        k = int(deg[v])
        if k >= 2:
            top = torch.topk(m[start:start + k], 2, dim=0).values
            worst = min(worst, float((top[0] - top[1]).min()))
        start += k
    return worst / float(msg.abs().max())


def condition_max(msg, dst, n):
    """Raises the largest message of every (destination, column) -- the lowest-numbered edge among equal ones -- by 1e-3 of the scale
    (in place, float32): its lead only grows."""
    E, D = msg.shape
    idx = dst.view(-1, 1).expand(-1, D)
    top = torch.full((n, D), float("-inf")).scatter_reduce(0, idx, msg, "amax", include_self=True)
    eid = torch.arange(E).view(-1, 1).expand(-1, D)
    first = torch.full((n, D), E).scatter_reduce(0, idx, torch.where(msg == top[dst], eid, torch.full_like(eid, E)), "amin", include_self=True)
    msg[eid == first[dst]] += 1e-3 * float(msg.abs().max())
    return msg


@functools.lru_cache(maxsize=8)
def rows_input(name, M, D, seed, std=1.0):
    """A seeded [M, D] float32 input, shared (and never modified) by the cases that ask for the same one."""
    return seeded(name, (M, D), seed, std)
