"""The GRU sequence pair (g2v_gru_seq_fwd / _bwd) restated in plain torch with the dtype as a parameter, the seeded inputs of its
float64 tests and their error bounds (tests/test_gru_ref_host.py on the host, tests/test_gpu_gru_f64.py on the GPU).  No device, no
library: the recurrence is the one of include/g2v.h (the comment above g2v_gru_dir), written out once more,

  r = s(gi_r + gh_r), z = s(gi_z + gh_z), n = tanh(gi_n + r gh_n), h' = (1 - z) n + z h,   gh = h W_hh^T + b_hh,

with pack_padded_sequence semantics under `lengths`: a row keeps its state where t >= length, its padded hs is zero, and the reverse
direction walks t = T-1 .. 0, so that a row's first live step is its own last one.  gates = r, z, n, gh_n.

The backward is AUTOGRAD on per-step leaves: every gi_t is a leaf and every gh_t keeps its gradient, so dgi_t / dgh_t are the
gradients of sum <hs, d_hs> + <h_n, d_hn_eff> with respect to exactly the two arrays the header names; dh0, dW_hh, db_hh are the
gradients of the leaves h0, W_hh, b_hh.  What lies behind gi is the chain written by hand, dx_t = dgi_t W_ih, dW_ih = sum dgi_t^T
x_t, db_ih = sum dgi_t (tests/test_gru_ref_host.py holds all of it to autograd through torch.nn.GRU).  d_hn_eff = d_hn, or with the
fused quantiser backward d_hn + gloss coef (z - q).

gi is an INPUT of the call (float32 values, x W_ih^T + b_ih rounded once) unless the projection is fused; then the restatement
forms it in `dtype` from x.  Packed and gathered are layouts of that one dense gi: row_off / pack / unpack / gather_layout.

The error measure is tests/_dec_ref.py's: per time step max|got_t - ref_t| / max|ref_t| (step_err), e32_t the float32 run against
the float64 run, bound_t = min(MARGIN max(e32_t, 2u), cap), MARGIN = 8, u = 2^-24; the caps are what test_gru_seq asserts over a
whole array, 2e-5 for hs, h_n, gates and 5e-5 for every gradient.  The GRU has no discontinuity (the length masks are inputs), so
nothing is excluded but what the header leaves undefined: gates rows at t >= length and packed dgi rows outside their sequences,
which `defined` zeroes on both sides."""
import functools
import math

import torch

import _dec_ref as R

U, MARGIN = R.U, R.MARGIN
CAP_FWD, CAP_GRAD = 2e-5, 5e-5
FWD_ARRAYS = ("hs", "h_n", "gates")
STEP_ARRAYS = ("hs", "gates", "dgi", "dgh", "dx")                       # leading axis = time
GRADS = ("dgi", "dgh", "dh0", "dx", "dw_hh", "db_hh", "dw_ih", "db_ih")
TABLE_ROWS = 57                                                          # of a gathered gi
HN_GLOSS, HN_COEF = 0.7, 0.37                                            # the quantiser term: order one beside d_hn


def inputs(T, B, H, ndir, seed, *, reverse=None, h0=False, lengths=False, gathered=False):
    """float32 / int CPU inputs of one case keyed by one seed; in_dim = H, weights scaled 1 / sqrt(H).  reverse: one flag per
    direction (default: forward, then reverse).  lengths: sorted descending with lengths[0] = T, as packed rows require."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    k, G = 1.0 / math.sqrt(H), 3 * H
    inp = {"T": T, "B": B, "H": H, "ndir": ndir, "reverse": tuple(reverse) if reverse is not None else (False, True)[:ndir]}
    inp["x"] = rn(T, B, H)
    inp["w_ih"], inp["w_hh"] = rn(ndir, G, H) * k, rn(ndir, G, H) * k
    inp["b_ih"], inp["b_hh"] = rn(ndir, G) * 0.1, rn(ndir, G) * 0.1
    inp["h0"] = rn(ndir, B, H) * 0.5 if h0 else None
    inp["lengths"] = None
    if lengths:
        ln = torch.randint(1, T + 1, (B,), generator=g).sort(descending=True).values
        ln[0] = T
        inp["lengths"] = ln.to(torch.int32)
    if gathered:      # the dense gi of a gathered call: every row is one of TABLE_ROWS
        table, idx = rn(ndir, TABLE_ROWS, G), torch.randint(0, TABLE_ROWS, (T * B,), generator=g)
        inp["gi"] = table[:, idx].reshape(ndir, T, B, G).contiguous()
    else:
        inp["gi"] = torch.stack([(inp["x"].reshape(T * B, H) @ inp["w_ih"][d].t() + inp["b_ih"][d]).reshape(T, B, G) for d in range(ndir)])
    inp["d_hs"], inp["d_hn"] = rn(ndir, T, B, H), rn(ndir, B, H)
    inp["hn_z"], inp["hn_q"] = rn(ndir, B, H), rn(ndir, B, H)
    return inp


def valid(inp):
    """(T, B) bool: position (t, b) lies inside its sequence"""
    T, B = inp["T"], inp["B"]
    if inp["lengths"] is None:
        return torch.ones(T, B, dtype=torch.bool)
    return inp["lengths"].long().unsqueeze(0) > torch.arange(T).unsqueeze(1)


def run(inp, dtype, *, fused=False, hn=False, grad=True):
    """Every array a device call writes, per direction, in `dtype` (list of dicts of detached tensors: hs, h_n, gates, and with
    grad the keys of GRADS).  fused: gi is formed here from x.  hn: the quantiser term is added to d_hn."""
    T, B, H, live = inp["T"], inp["B"], inp["H"], valid(inp)
    out = []
    for d in range(inp["ndir"]):
        w_hh = inp["w_hh"][d].to(dtype).clone().requires_grad_(grad)
        b_hh = inp["b_hh"][d].to(dtype).clone().requires_grad_(grad)
        w_ih, b_ih, x = inp["w_ih"][d].to(dtype), inp["b_ih"][d].to(dtype), inp["x"].to(dtype)
        h0 = (inp["h0"][d].to(dtype) if inp["h0"] is not None else torch.zeros(B, H, dtype=dtype)).clone().requires_grad_(grad)
        gi_all = (x.reshape(T * B, H) @ w_ih.t() + b_ih).reshape(T, B, 3 * H) if fused else inp["gi"][d].to(dtype)
        gis, ghs, hs, gates, h = [None] * T, [None] * T, [None] * T, [None] * T, h0
        with torch.set_grad_enabled(grad):
            for t in (range(T - 1, -1, -1) if inp["reverse"][d] else range(T)):
                gi = gi_all[t].detach().clone().requires_grad_(grad)
                gh = h @ w_hh.t() + b_hh
                if grad:
                    gh.retain_grad()
                r = torch.sigmoid(gi[:, :H] + gh[:, :H])
                z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
                n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
                hnew, m = (1 - z) * n + z * h, live[t].unsqueeze(1)
                h = torch.where(m, hnew, h)                                # rows freeze after their last step
                hs[t] = torch.where(m, hnew, torch.zeros_like(hnew))       # padded outputs are zero
                gates[t] = torch.where(m, torch.cat([r, z, n, gh[:, 2 * H:]], dim=1), torch.zeros(B, 4 * H, dtype=dtype))
                gis[t], ghs[t] = gi, gh
            hs_all = torch.stack(hs)
            res = {"hs": hs_all.detach(), "h_n": h.detach(), "gates": torch.stack(gates).detach()}
            if grad:
                d_hn = inp["d_hn"][d].to(dtype)
                if hn:
                    d_hn = d_hn + HN_GLOSS * HN_COEF * (inp["hn_z"][d].to(dtype) - inp["hn_q"][d].to(dtype))
                ((hs_all * inp["d_hs"][d].to(dtype)).sum() + (h * d_hn).sum()).backward()
        if grad:
            zg = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
            dgi = torch.stack([zg(t) for t in gis])
            res.update(dgi=dgi, dgh=torch.stack([zg(t) for t in ghs]), dh0=zg(h0), dw_hh=zg(w_hh), db_hh=zg(b_hh))
            res["dx"] = (dgi.reshape(T * B, 3 * H) @ w_ih).reshape(T, B, H)
            res["dw_ih"] = dgi.reshape(T * B, 3 * H).t() @ x.reshape(T * B, H)
            res["db_ih"] = dgi.sum(dim=(0, 1))
        out.append(res)
    return out


# ---------------------------------------------------------------------------------------------------------------- layouts of gi
def row_off(inp):
    """the T packed row offsets: off[t] = n_0 + .. + n_{t-1}, n_t = #{lengths > t}"""
    n = valid(inp).sum(1).tolist()
    return [sum(n[:t]) for t in range(inp["T"])]


def pack(dense, inp):
    """(T, B, C) -> (sum(lengths), C): the positions inside their sequences, step-major (lengths sorted descending)"""
    n = valid(inp).sum(1).tolist()
    return torch.cat([dense[t, :n[t]] for t in range(inp["T"])], dim=0).contiguous()


def unpack(packed, inp, fill=0.0):
    """the inverse of pack: (T, B, C) with `fill` outside the sequences"""
    n, off = valid(inp).sum(1).tolist(), row_off(inp)
    dense = torch.full((inp["T"], inp["B"], packed.shape[-1]), fill, dtype=packed.dtype)
    for t in range(inp["T"]):
        dense[t, :n[t]] = packed[off[t]:off[t] + n[t]]
    return dense


def gather_layout(gi, inp, packed=False):
    """table (V, 3H) and int64 index of a dense gi whose rows repeat: gi row r of the (packed) layout = table[index[r]]"""
    T, B = inp["T"], inp["B"]
    table, inverse = torch.unique(gi.reshape(T * B, -1), dim=0, return_inverse=True)
    index = inverse.reshape(T, B, 1)
    index = pack(index, inp) if packed else index
    return table.contiguous(), index.reshape(-1).contiguous()


# ---------------------------------------------------------------------------------------------------------------- error measure
def _steps_of(name):
    """the array of tests/_dec_ref.py with this array's time axis: per time step for STEP_ARRAYS, one step for the rest"""
    return "y" if name in STEP_ARRAYS else "dh_init"


def step_err(got, ref, name):
    return R.step_err(got, ref, _steps_of(name))


def cap_of(name):
    return CAP_FWD if name in FWD_ARRAYS else CAP_GRAD


def defined(name, t, inp, packed=False):
    """`t` with the positions the header leaves undefined set to zero: gates rows at t >= length, and for a packed call the dgi
    rows outside their sequences (which do not exist in its array).  Everything else is returned as it is."""
    if name == "gates" or (name == "dgi" and packed):
        return torch.where(valid(inp).unsqueeze(2), t, torch.zeros_like(t))
    return t


def check(label, name, got, ref, e32):
    """tests/_dec_ref.py check under this file's caps: prints the worst step's e_kernel, e32, their ratio and the bound, returns
    (ok, line, ratio)"""
    return R.check(label, name, got, ref, e32, cap=cap_of(name), steps_of=_steps_of(name))


# --------------------------------------------------------------------------------------------------------------- a case's reference
def case_key(case):
    return (case["T"], case["B"], case["H"], case["ndir"], case["seed"], tuple(case["reverse"]) if case.get("reverse") else None,
            bool(case.get("h0")), bool(case.get("lengths")), bool(case.get("gathered")), bool(case.get("fused")), bool(case.get("hn")),
            bool(case.get("bwd", True)))


@functools.lru_cache(maxsize=2)
def _reference(key):
    T, B, H, ndir, seed, reverse, h0, lengths, gathered, fused, hn, bwd = key
    inp = inputs(T, B, H, ndir, seed, reverse=reverse, h0=h0, lengths=lengths, gathered=gathered)
    f64, f32 = run(inp, torch.float64, fused=fused, hn=hn, grad=bwd), run(inp, torch.float32, fused=fused, hn=hn, grad=bwd)
    names = FWD_ARRAYS + (GRADS if bwd else ())
    return {"inp": inp, "f64": f64, "f32": f32, "e32": [{k: step_err(a[k], b[k], k) for k in names} for a, b in zip(f32, f64)]}


def reference(case):
    """inputs, the float64 and float32 runs and e32 per direction, array and step of one case of GRU_F64_CASES; the last two stay
    cached (padded gates and gradients are already zero on both sides: run() writes them so)"""
    return _reference(case_key(case))
