"""g2v_attn_code_rollout_fwd / _bwd and g2v_code_cluster_bptt (csrc/t2e_rollout.hip: code_step_fwd_kernel, code_cluster_fwd_kernel,
code_bptt_kernel + code_bn_bwd_apply_kernel, code_step_bwd_att_kernel, code_cluster_bptt_kernel) against the float64 restatement of
tests/_code_ref.py on every route the entries take, at the shapes of CODE_F64_CASES (tests/_t2e_route_shapes.py).  Every saved
array and every gradient is compared on its own, per time step: e_kernel_t <= min(8 max(e32_t, 2u), cap), all of it from the
reference alone; the fed codes must equal the float64 run's exactly, every row (tests/_code_ref.py says how the two
discontinuities, ReLU and the greedy argmax, are handled).  Each case prints, per array, the worst step's e_kernel, e32, their ratio
and the bound.

Largest figures on the MI355X per route and array, over all cases of the route: e_kernel / max(e32, 2u) (the quantity the margin
of 8 multiplies), then e_kernel and e32 of that step.  STEP: code_step_fwd_kernel, and code_bptt_kernel with its batched tail (also
behind a CLUSTER forward); STEP*1: the attention cases, forward and code_step_bwd_att_kernel; CLUSTER: code_cluster_fwd_kernel; BPTT:
g2v_code_cluster_bptt by itself; unal.: the calls whose element-wise arrays are unaligned, all three entries:
               STEP                    STEP*1                  CLUSTER                 BPTT                    unal.
  ec           0.00 0.0e+00 0.0e+00    0.40 4.8e-08 6.7e-08    0.00 0.0e+00 0.0e+00    -                       0.31 3.7e-08 3.7e-08
  u            2.00 4.0e-07 2.0e-07    3.46 9.1e-07 2.6e-07    1.15 1.5e-07 1.3e-07    -                       1.15 1.5e-07 1.3e-07
  h0           2.42 4.4e-07 1.8e-07    2.03 3.6e-07 1.8e-07    1.64 3.3e-07 2.0e-07    -                       1.36 2.2e-07 1.7e-07
  h1           1.65 2.0e-07 1.2e-07    1.91 2.8e-07 1.5e-07    2.38 3.8e-07 1.6e-07    -                       1.73 2.3e-07 1.3e-07
  logits       2.42 5.4e-07 2.2e-07    2.44 3.9e-07 1.6e-07    1.44 1.7e-07 1.2e-07    -                       1.50 2.2e-07 1.5e-07
  a            2.07 4.3e-07 2.1e-07    2.57 6.7e-07 2.6e-07    1.27 1.7e-07 1.3e-07    -                       1.26 2.9e-07 2.3e-07
  bn_stats     1.81 2.2e-07 1.2e-07    2.46 4.2e-07 1.7e-07    1.22 1.8e-07 1.5e-07    -                       1.33 1.6e-07 1.0e-07
  gates0       1.82 6.1e-07 3.3e-07    1.75 6.3e-07 3.6e-07    2.03 6.8e-07 3.3e-07    -                       1.30 2.6e-07 2.0e-07
  gates1       2.16 5.1e-07 2.3e-07    1.95 5.0e-07 2.6e-07    2.09 5.5e-07 2.6e-07    -                       1.58 2.3e-07 1.5e-07
  running_mean 1.00 1.4e-07 1.4e-07    1.26 1.5e-07 1.2e-07    1.27 1.5e-07 8.0e-08    -                       1.00 1.2e-07 1.2e-07
  running_var  1.20 1.4e-07 8.8e-08    1.15 1.6e-07 1.3e-07    1.30 1.7e-07 1.3e-07    -                       1.18 2.1e-07 1.8e-07
  d_hidden0    2.90 6.7e-07 2.3e-07    1.25 3.8e-07 3.0e-07    -                       1.51 1.8e-07 8.2e-08    1.18 1.7e-07 1.4e-07
  d_bn_b       1.96 3.5e-07 1.8e-07    1.78 5.9e-07 3.3e-07    -                       -                       1.47 2.1e-07 1.5e-07
  d_w_ih0      1.83 7.3e-07 4.0e-07    1.68 7.2e-07 4.3e-07    -                       -                       1.17 2.7e-07 2.3e-07
  d_w_hh0      2.29 7.2e-07 3.2e-07    1.69 4.9e-07 2.9e-07    -                       -                       1.25 1.9e-07 1.5e-07
  d_b_ih0      1.83 1.1e-06 5.8e-07    1.43 5.9e-07 4.1e-07    -                       -                       1.19 1.6e-07 1.3e-07
  d_b_hh0      2.12 6.3e-07 3.0e-07    1.76 6.3e-07 3.6e-07    -                       -                       1.33 1.6e-07 1.1e-07
  d_w_ih1      2.11 6.0e-07 2.8e-07    1.49 5.5e-07 3.7e-07    -                       -                       1.08 1.3e-07 1.2e-07
  d_w_hh1      2.84 6.6e-07 2.3e-07    1.27 5.2e-07 4.1e-07    -                       -                       1.04 2.3e-07 2.2e-07
  d_b_ih1      2.24 3.8e-07 1.7e-07    1.78 4.8e-07 2.7e-07    -                       -                       1.11 1.9e-07 1.7e-07
  d_b_hh1      2.80 4.4e-07 1.6e-07    1.26 4.1e-07 3.2e-07    -                       -                       1.48 1.8e-07 9.4e-08
  d_w_out      1.71 2.4e-07 1.4e-07    1.65 2.4e-07 1.4e-07    -                       -                       1.53 2.8e-07 1.8e-07
  d_b_out      0.99 1.2e-07 1.1e-07    1.26 1.5e-07 7.6e-08    -                       -                       0.94 1.1e-07 6.2e-08
  d_emb        2.20 9.9e-07 4.5e-07    1.39 6.8e-07 4.9e-07    -                       -                       1.20 3.3e-07 2.7e-07
  d_w_pre      1.94 6.0e-07 3.1e-07    1.20 5.6e-07 4.6e-07    -                       -                       1.02 2.5e-07 2.4e-07
  d_bn_w       1.75 7.5e-07 4.3e-07    1.48 5.4e-07 3.7e-07    -                       -                       1.07 3.0e-07 2.8e-07
  x1           1.78 3.1e-07 1.7e-07    1.48 3.2e-07 2.2e-07    1.41 2.3e-07 1.7e-07    -                       1.19 2.0e-07 1.7e-07
  hp           -                       1.64 2.9e-07 1.8e-07    -                       -                       1.64 2.9e-07 1.8e-07
  attw         -                       2.42 2.9e-07 1.2e-07    -                       -                       0.96 1.1e-07 8.3e-08
  d_w_attn     -                       0.91 3.6e-07 3.9e-07    -                       -                       0.91 3.6e-07 3.9e-07
  d_b_attn     -                       2.01 1.2e-06 6.0e-07    -                       -                       1.00 7.6e-07 7.6e-07
  d_v_attn     -                       1.40 6.6e-07 4.7e-07    -                       -                       0.95 2.7e-07 2.8e-07
  d_enc        -                       1.28 2.9e-07 2.3e-07    -                       -                       1.12 4.1e-07 3.6e-07
  dgi0         -                       -                       -                       0.99 2.2e-07 2.2e-07    0.96 2.5e-07 2.6e-07
  dgh0         -                       -                       -                       1.34 2.8e-07 2.1e-07    1.08 2.5e-07 2.4e-07
  dgi1         -                       -                       -                       1.16 2.8e-07 2.4e-07    0.94 1.6e-07 1.7e-07
  dgh1         -                       -                       -                       1.34 2.8e-07 2.0e-07    1.01 1.7e-07 1.7e-07
  da           -                       -                       -                       1.00 1.8e-07 1.8e-07    0.90 1.7e-07 1.9e-07

Largest ratio: 3.46 (u of STEP-24x200x512xTw64-tw-max, STEP*1).
Nothing comes near the margin.  d_b_pre (zero in the reference, it feeds BatchNorm) stayed below 3e-8 against bounds of 2e-7 to
4e-7; the fed codes equalled the float64 run's in every row of every case, and both tie cases fed the lower code.

One thing the first device run showed: bn_stats of the one-row case stood at 2e-3.  At B = 1 the variance is 0, but the kernels'
s2 / B - mv * mv is contracted to a fused multiply-add and leaves the rounding residue of mv^2, up to u c^2, which against eps =
1e-5 moves 1 / sqrt(var + eps) by that much at |c| of a few.  Both forward kernels now take the variance of one row as 0
(bn_batch_var, csrc/t2e_rollout.hip); from two rows on nothing changed.

Alignment, read out of the code before any unaligned call was run (include/g2v.h states the contract):
  * g2v_attn_code_rollout_fwd refused h_init, enc, enc_proj, emb, the biases, bn_w / bn_b, v_attn, the masks and the saved arrays it
    moves as float4s, but not w_pre, w_ih*, w_hh* and w_out: the step kernels read those through launch_pack, element by element,
    while code_cluster_fwd_kernel loads its rows of them as float4s.  They are refused now.  Served at 4 bytes, element-wise on both
    routes: w_attn, bn_running_mean / _var, bn_stats, attw (and codes / ids, one int64 at a time).
  * g2v_attn_code_rollout_bwd refused only workspace, d_logits and d_hidden0, yet code_bptt_kernel, code_bn_bwd_apply_kernel and
    code_step_bwd_att_kernel read u, a, bn_stats, h0, h1, the gates, hp, bn_w, v_attn, enc and enc_proj as float4s and the masks
    as words of four flags, and write d_enc as float4s; the dense tail takes w_pre, ids, ec, x1 and every gradient array at widths
    of its own.  All of them are refused now.  Served at 4 bytes: w_ih*, w_hh*, w_out, w_attn (launch_pack, code_split_cols_kernel).
  * g2v_code_cluster_bptt already refused every array its kernel moves as float4s; w_ih* and w_hh* it reads element-wise.
"""
import pytest
import torch

import _code_ref as C
from _dev_arrays import Arrays as _Arrays
from _t2e_route_shapes import CODE_F64_CASES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
GATE_MATS = ("w_ih0", "w_hh0", "w_ih1", "w_hh1")
FWD_SERVED = frozenset(("codes", "ids", "w_attn", "bn_running_mean", "bn_running_var", "bn_stats", "attw"))
BWD_SERVED = frozenset(GATE_MATS + ("w_out", "w_attn"))
BPTT_SERVED = frozenset(GATE_MATS)
_CASES = {c["id"]: c for c in CODE_F64_CASES}
UNALIGNED = ("STEP-24x48x40xTw5-plain", "STEP-33x48x40-drop", "CLUSTER-16x48x40-drop")
assert set(UNALIGNED) <= set(_CASES)


@pytest.fixture(scope="module")
def ops():
    from gesture2vec_amd import _lib, ops as o
    assert _lib.load().g2v_device_ok() == 1, "no gfx950 device visible"
    return o


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else t.dtype)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


class _Put:
    """device arrays of one call: the names in `off` 4 bytes (masks: 1 byte, int64: 8 bytes) past a 16-byte boundary"""

    def __init__(self, off=frozenset()):
        self.off, self.al, self.un = frozenset(off), _Arrays(False), _Arrays(True)

    def put(self, name, src):
        return None if src is None else (self.un if name in self.off else self.al).put(src)

    def full(self, name, shape, value=NAN, dtype=torch.float32):
        return (self.un if name in self.off else self.al).full(shape, value, dtype)


def _weights(inp, mk, running=True):
    wt = {k: mk.put(k, v) for k, v in inp["w"].items()}
    wt["bn_running_mean"] = mk.put("bn_running_mean", inp["running_mean"]) if running else None
    wt["bn_running_var"] = mk.put("bn_running_var", inp["running_var"]) if running else None
    return wt


def _inputs(inp, mk, case):
    return {"codes": mk.put("codes", inp["codes"]), "h_init": mk.put("h_init", inp["h_init"]), "enc": mk.put("enc", inp["enc"]),
            "enc_proj": mk.put("enc_proj", inp["enc_proj"]), "keep_emb": mk.put("keep_emb", inp["keep_emb"]) if case["emb_drop"] else None,
            "keep_l0": mk.put("keep_l0", inp["keep_l0"]), "d_logits": mk.put("d_logits", inp["d_logits"]),
            "dh_top": mk.put("dh_top", inp["dh_top"])}


def _saved(case, ops, mk):
    S1, B, H, K, Tw, att, training = case["S1"], case["B"], case["H"], case["K"], case["Tw"], case["att"], case["training"]
    Hin = 2 * H if att else H
    f = lambda name, *s: mk.full(name, s)
    sv = {"ids": mk.full("ids", (S1, B), -1, torch.int64), "ec": f("ec", S1, B, Hin), "u": f("u", S1, B, H), "h0": f("h0", S1 + 1, B, H),
          "h1": f("h1", S1 + 1, B, H), "logits": f("logits", S1, B, K), "bn_partial": f("bn_partial", 2, (B + 15) // 16, 2, H)}
    if training:      # eval mode: the optional saved arrays stay NULL
        sv.update(a=f("a", S1, B, H), bn_stats=f("bn_stats", S1, 2, H), gates0=f("gates0", S1, B, 4 * H), gates1=f("gates1", S1, B, 4 * H),
                  x1=f("x1", S1, B, H) if case["p"] > 0 else None)
    if att:
        sv.update(hp=f("hp", S1, B, H), attw=f("attw", S1, B, Tw))
    return sv


def _forward(ops, case, inp, off=frozenset(), running=True):
    mk = _Put(off)
    wt, dev, sv = _weights(inp, mk, running), _inputs(inp, mk, case), _saved(case, ops, mk)
    ops.code_rollout_fwd(dev["codes"], dev["h_init"], dev["enc"], dev["enc_proj"], wt, sv, dev["keep_emb"], dev["keep_l0"], case["p"],
                         case["n_pre"], case["training"], case["S1"], case["B"], case["H"], case["K"], case["Tw"])
    torch.cuda.synchronize()
    return sv, wt, dev


def _grads(case, mk):
    B, H, K, G, att = case["B"], case["H"], case["K"], 3 * case["H"], case["att"]
    shapes = {"d_hidden0": (2, B, H), "d_emb": (K, H), "d_w_pre": (H, 2 * H if att else H), "d_b_pre": (H,), "d_bn_w": (H,), "d_bn_b": (H,),
              "d_w_out": (K, H), "d_b_out": (K,)}
    for l in (0, 1):
        shapes.update({f"d_w_ih{l}": (G, H), f"d_w_hh{l}": (G, H), f"d_b_ih{l}": (G,), f"d_b_hh{l}": (G,)})
    if att:
        shapes.update(d_w_attn=(H, 2 * H), d_b_attn=(H,), d_v_attn=(H,), d_enc=(case["Tw"], B, H))
    return {k: mk.full(k, s) for k, s in shapes.items()}


def _backward(ops, case, inp, sv, off=frozenset()):
    mk = _Put(off)
    wt, dev, gr = _weights(inp, mk), _inputs(inp, mk, case), _grads(case, mk)
    ops.code_rollout_bwd(dev["d_logits"], dev["enc"], dev["enc_proj"], wt, {k: v for k, v in sv.items() if k != "logits"}, gr,
                         dev["keep_emb"], dev["keep_l0"], case["p"], case["S1"], case["B"], case["H"], case["K"], case["Tw"])
    torch.cuda.synchronize()
    return gr


def _bptt(ops, case, inp, sv, off=frozenset()):
    S1, B, H = case["S1"], case["B"], case["H"]
    mk = _Put(off)
    wt, dev = _weights(inp, mk), _inputs(inp, mk, case)
    out = {k: mk.full(k, (S1, B, 3 * H)) for k in ("dgi0", "dgh0", "dgi1", "dgh1")}
    out.update(da=mk.full("da", (S1, B, H)), d_hidden0=mk.full("d_hidden0", (2, B, H)))
    ops.code_cluster_bptt(dev["dh_top"], wt, sv, dev["keep_l0"], case["p"], S1, B, H, out=tuple(out.values()))
    torch.cuda.synchronize()
    return out


def _run(ops, case, off_fwd=frozenset(), off_bwd=frozenset(), off_bptt=frozenset(), tag=""):
    from gesture2vec_amd import _lib
    lib = _lib.load()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus != 256:
        pytest.skip(f"CODE_F64_CASES names the routes of a device with 256 CUs; this one has {cus}")
    S1, B, H, K, Tw, att, training = case["S1"], case["B"], case["H"], case["K"], case["Tw"], case["att"], case["training"]
    ref = C.reference(case)
    inp, f64, e32, label = ref["inp"], ref["f64"], ref["e32"], case["id"] + tag
    bad = []

    def held(name, got, want, route):
        if name not in e32:      # the reference is exactly zero and so is its float32 restatement: nothing else is within the bound
            ok, line = not bool((_bits(got.float()) << 1).any()), f"{label} {route} {name}: reference exactly zero"
            print(line)
        else:
            ok, line, _ = C.check(f"{label} {route}", name, got.cpu(), want, e32[name], cap=C.cap_of(name), steps_of=C.steps_of(name))
        if not ok:
            bad.append(line)

    with _lib.Context.current().scoped(persistent=case["level"]):
        rt = dict(facts=("ENTRY",), persistent=-1, cus=0)
        assert ops.code_route(S1, B, H, K, Tw, att, backward=False, **rt) == case["route"]
        if training:
            assert ops.code_route(S1, B, H, K, Tw, att, backward=True, **rt) == case["route_bwd"]
        assert lib.g2v_dec_rollout_persist_fault(0) == 0
        # ---------------------------------------------------------------------------------------------------------- forward
        sv, wt, _ = _forward(ops, case, inp, off_fwd)
        assert lib.g2v_dec_rollout_persist_fault(0) == 0, "a bounded wait of the forward ran out"
        names = C.fwd_names(case)
        for name in names:
            assert not torch.isnan(sv[name]).any(), f"{name}: the forward left part of it unwritten"
        assert torch.equal(sv["ids"].cpu(), f64["ids"]), (
            f"{int((sv['ids'].cpu() != f64['ids']).sum())} fed codes differ from the float64 run's (argmax gap {ref['gap_min']:.2e}, "
            f"tau_arg {ref['tau_arg']:.2e})")
        for name in names:
            held(name, sv[name], f64[name], case["route"])
        assert _same(sv["h0"][0].cpu(), inp["h_init"][0]) and _same(sv["h1"][0].cpu(), inp["h_init"][1]), "slot 0 of h0 / h1 is h_init"
        for k in ("running_mean", "running_var"):
            if training:
                held(k, wt["bn_" + k], f64[k], case["route"])
            else:
                assert _same(wt["bn_" + k].cpu(), inp[k]), f"eval mode touched {k}"
        assert not bad, "\n".join(bad)
        sv2, wt2, _ = _forward(ops, case, inp)
        for k in names + ["ids"]:
            assert _same(sv[k], sv2[k]), f"two forwards differ: {k}"
        assert _same(wt["bn_running_mean"], wt2["bn_running_mean"]) and _same(wt["bn_running_var"], wt2["bn_running_var"])
        if case["deferred"]:      # bn_running_mean = bn_running_var = NULL, then the deferred commit on bn_stats
            sv3, _, _ = _forward(ops, case, inp, running=False)      # (aligned: the commit is another entry's kernel)
            for k in names:
                assert _same(sv[k], sv3[k]), f"a forward without running statistics differs: {k}"
            mk = _Put()
            rm, rvar = mk.put("bn_running_mean", inp["running_mean"]), mk.put("bn_running_var", inp["running_var"])
            ops.bn_running_update_invstd(sv3["bn_stats"], sv3["bn_stats"].view(-1)[H:], 2 * H, rm, rvar, S1, H, B)
            torch.cuda.synchronize()
            held("running_mean", rm, f64["running_mean"], "deferred")
            held("running_var", rvar, f64["running_var"], "deferred")
            assert not bad, "deferred commit\n" + "\n".join(bad)
        if not training:
            return
        # --------------------------------------------------------------------------------------------------------- backward
        g64, differs = C.grad_reference(case, sv2["a"])
        assert differs == 0, f"{differs} ReLU decisions differ from float64 away from zero"
        gr = _backward(ops, case, inp, sv2, off_bwd)
        gnames = C.grad_names(att)
        for name in gnames:
            assert not torch.isnan(gr[name]).any(), f"{name}: NaN (unwritten)"
        # b_pre feeds BatchNorm: its gradient is zero in the reference, and at B = 1 so is du with all that derives from it
        w_pre, bn_w = inp["w"]["w_pre"].double(), float(inp["w"]["bn_w"].abs().max())
        if B == 1:      # what is left is the rounding of xhat = (u - mean) invstd and of dbn - sum(dbn) / B
            lim_du = C.MARGIN * 2 * C.U * float(g64["dbn"].abs().max()) * bn_w / C.EPS ** 0.5
            special = {"d_b_pre": S1 * lim_du, "d_w_pre": S1 * lim_du * float(f64["ec"].abs().max()),
                       "d_emb": S1 * lim_du * 2 * float(w_pre.abs().sum(0).max())}
        else:
            t32, t64 = ref["g32_d_b_pre"], 2 * C.U * float(g64["du"].abs().sum(dim=(0, 1)).max())
            print(f"{label} d_b_pre: float32 restatement {t32:.3e}  2u max_f sum|du64| {t64:.3e}")
            special = {"d_b_pre": C.MARGIN * max(t32, t64)}
        for name in gnames:
            if name in special:
                got = float(gr[name].abs().max())
                print(f"{label} {case['route_bwd']} {name}: max {got:.3e}  bound {special[name]:.3e} (reference exactly zero)")
                if not got <= special[name]:
                    bad.append(f"{name}: {got:.3e} > {special[name]:.3e}")
            else:
                held(name, gr[name], g64[name], case["route_bwd"])
        unfed = torch.ones(K, dtype=torch.bool)
        unfed[f64["ids"].reshape(-1)] = False
        assert not bool((_bits(gr["d_emb"].cpu())[unfed] != 0).any()), "d_emb: a row whose code was never fed is not bitwise zero"
        assert not bad, "\n".join(bad)
        gr2 = _backward(ops, case, inp, sv2)
        for k in gnames:
            assert _same(gr[k], gr2[k]), f"two backwards differ: {k}"
        if not case["bptt"]:
            return
        # ------------------------------------------------------------------------------------------- the cluster BPTT by itself
        assert ops.code_route(S1, B, H, K, Tw, att, backward=2, **rt) == "CLUSTER"
        out = _bptt(ops, case, inp, sv2, off_bptt)
        assert lib.g2v_dec_rollout_persist_fault(0) == 0, "a bounded wait of the cluster BPTT ran out"
        for name, got in out.items():
            assert not torch.isnan(got).any(), f"{name}: the cluster BPTT left part of it unwritten"
            held(name, got, g64[name], "BPTT")
        assert not bad, "\n".join(bad)
        out2 = _bptt(ops, case, inp, sv2)
        assert lib.g2v_dec_rollout_persist_fault(0) == 0
        for k in out:
            assert _same(out[k], out2[k]), f"two cluster BPTTs differ: {k}"


@pytest.mark.parametrize("case", CODE_F64_CASES, ids=lambda c: c["id"])
def test_code_rollout_matches_float64_on_its_route(ops, case):
    _run(ops, case)


def test_a_tie_feeds_the_lowest_index(ops):
    """codes k1 < k2 with identical rows of w_out, b_out and emb: their logits are bitwise equal on the device and k1 is fed
    (the tie cases themselves run above; this states what they rely on)"""
    for case in (c for c in CODE_F64_CASES if c["tie"] is not None):
        from gesture2vec_amd import _lib
        k1, k2 = case["tie"][:2]
        ref = C.reference(case)
        with _lib.Context.current().scoped(persistent=case["level"]):
            sv, _, _ = _forward(ops, case, ref["inp"])
        lg, ids, free = sv["logits"].cpu(), sv["ids"].cpu(), ref["f64"]["free"]
        assert _same(lg[..., k1], lg[..., k2]), case["id"]
        assert int((ids[free] == k1).sum()) * 4 >= ids[free].numel() and not bool((ids[free] == k2).any()), case["id"]
        top = lg[:-1][free[1:]].max(-1).values
        assert bool((top == lg[:-1][free[1:]][..., k1]).any()), "no row whose maximum is the tied pair"


@pytest.mark.parametrize("cid", UNALIGNED)
def test_arrays_the_entries_serve_unaligned_meet_the_same_bounds(ops, cid):
    """every array an entry moves element-wise 4 bytes (int64: 8) past a 16-byte boundary; the results are bitwise those of the
    aligned call (asserted inside: the second forward / backward / BPTT of _run is aligned)"""
    case = _CASES[cid]
    _run(ops, case, FWD_SERVED, BWD_SERVED, BPTT_SERVED, tag="-unaligned")


_REFUSED_FWD = ("h_init", "w_pre", "w_ih0", "w_hh1", "w_out", "emb", "b_out", "u", "a", "gates1", "logits", "keep_emb", "keep_l0")
_REFUSED_BWD = ("d_logits", "w_pre", "bn_w", "ids", "ec", "u", "a", "bn_stats", "h1", "x1", "gates0", "keep_emb", "keep_l0", "d_emb",
                "d_w_hh0", "d_b_out", "d_hidden0")
_REFUSED_BWD_ATT = ("enc", "enc_proj", "v_attn", "hp", "attw", "d_w_attn", "d_enc")
_REFUSED_BPTT = ("dh_top", "keep_l0", "dgi0", "dgh1", "da", "d_hidden0", "gates0", "gates1", "h0", "h1")


def _untouched(arrays):
    return all(bool(torch.isnan(t).all()) for t in arrays if t is not None and t.is_floating_point())


def test_unaligned_arrays_the_kernels_move_in_vectors_are_refused(ops):
    """one array at a time 4 bytes (masks: 1 byte, ids: 8 bytes) off: the entry returns the error before any launch and every
    NaN-filled output stays NaN"""
    from gesture2vec_amd import _lib
    err = (_lib.G2VLibraryError, RuntimeError)
    for cid, bwd_names in (("STEP-33x48x40-drop", _REFUSED_BWD), ("STEP-24x48x40xTw5-plain", _REFUSED_BWD_ATT)):
        case = _CASES[cid]
        inp = C.reference(case)["inp"]
        with _lib.Context.current().scoped(persistent=case["level"]):
            sv, _, _ = _forward(ops, case, inp)
            for name in (_REFUSED_FWD if not case["att"] else ("enc", "enc_proj", "b_attn", "v_attn", "hp")):
                mk = _Put({name})
                wt, dev, s = _weights(inp, mk), _inputs(inp, mk, case), _saved(case, ops, mk)
                with pytest.raises(err, match="16-byte alignment"):
                    ops.code_rollout_fwd(dev["codes"], dev["h_init"], dev["enc"], dev["enc_proj"], wt, s, dev["keep_emb"], dev["keep_l0"],
                                         case["p"], case["n_pre"], True, case["S1"], case["B"], case["H"], case["K"], case["Tw"])
                torch.cuda.synchronize()
                assert _untouched(s.values()) and bool((s["ids"] == -1).all()), f"forward, {name} unaligned: an output was written"
            for name in bwd_names:
                mk = _Put({name})
                wt, dev, gr = _weights(inp, mk), _inputs(inp, mk, case), _grads(case, mk)
                s = {k: (mk.put(k, v.cpu()) if k == name else v) for k, v in sv.items() if k != "logits"}
                with pytest.raises(err, match="16-byte alignment"):
                    ops.code_rollout_bwd(dev["d_logits"], dev["enc"], dev["enc_proj"], wt, s, gr, dev["keep_emb"], dev["keep_l0"], case["p"],
                                         case["S1"], case["B"], case["H"], case["K"], case["Tw"])
                torch.cuda.synchronize()
                assert _untouched(gr.values()), f"backward, {name} unaligned: an output was written"
    case = _CASES["CLUSTER-16x48x40-drop"]
    inp = C.reference(case)["inp"]
    S1, B, H = case["S1"], case["B"], case["H"]
    with _lib.Context.current().scoped(persistent=case["level"]):
        sv, _, _ = _forward(ops, case, inp)
        for name in _REFUSED_BPTT:
            mk = _Put({name})
            wt, dev = _weights(inp, mk), _inputs(inp, mk, case)
            out = {k: mk.full(k, (S1, B, 3 * H)) for k in ("dgi0", "dgh0", "dgi1", "dgh1")}
            out.update(da=mk.full("da", (S1, B, H)), d_hidden0=mk.full("d_hidden0", (2, B, H)))
            s = {k: (mk.put(k, v.cpu()) if k == name else v) for k, v in sv.items()}
            with pytest.raises(err, match="16-byte alignment"):
                ops.code_cluster_bptt(dev["dh_top"], wt, s, dev["keep_l0"], case["p"], S1, B, H, out=tuple(out.values()))
            torch.cuda.synchronize()
            assert _untouched(out.values()), f"cluster BPTT, {name} unaligned: an output was written"
        assert _lib.load().g2v_dec_rollout_persist_fault(0) == 0
