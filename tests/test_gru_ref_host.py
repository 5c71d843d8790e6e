"""CPU-only: the restatement of the GRU sequence pair (tests/_gru_ref.py) against torch.nn.GRU in float64 and the oracle's
gru_direction in float32, the consistency of its dgi / dgh with the weight gradients, its check function on planted defects, and the
conditions every case of GRU_F64_CASES (tests/_gru_route_shapes.py) must meet before tests/test_gpu_gru_f64.py may hold a kernel
to it: the named route in both directions of travel and every bound under its cap.  No kernel is launched."""
import pytest
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

import _gru_ref as G
import _gru_route_shapes as GS
from oracle import g2v_oracle as O


def _nn_gru(inp):
    """torch.nn.GRU in float64 on the inputs of one case (one layer, in_dim = H): hs and h_n per direction, and by autograd of
    sum <hs, d_hs> + <h_n, d_hn> the gradients of every parameter, of x and of h0"""
    T, B, H, ndir = inp["T"], inp["B"], inp["H"], inp["ndir"]
    gru = torch.nn.GRU(H, H, 1, bidirectional=ndir == 2).double()
    with torch.no_grad():
        for d in range(ndir):
            sfx = "_reverse" if d else ""
            for name, key in (("weight_ih_l0", "w_ih"), ("weight_hh_l0", "w_hh"), ("bias_ih_l0", "b_ih"), ("bias_hh_l0", "b_hh")):
                getattr(gru, name + sfx).copy_(inp[key][d].double())
    x = inp["x"].double().clone().requires_grad_(True)
    h0 = (inp["h0"].double() if inp["h0"] is not None else torch.zeros(ndir, B, H, dtype=torch.float64)).clone().requires_grad_(True)
    if inp["lengths"] is not None:
        out, h_n = gru(pack_padded_sequence(x, inp["lengths"].long(), enforce_sorted=True), h0 if inp["h0"] is not None else None)
        out, _ = pad_packed_sequence(out, total_length=T)
    else:
        out, h_n = gru(x, h0 if inp["h0"] is not None else None)
    hs = [out[:, :, d * H:(d + 1) * H] for d in range(ndir)]
    loss = sum((hs[d] * inp["d_hs"][d].double()).sum() + (h_n[d] * inp["d_hn"][d].double()).sum() for d in range(ndir))
    loss.backward()
    res = []
    for d in range(ndir):
        sfx = "_reverse" if d else ""
        res.append({"hs": hs[d].detach(), "h_n": h_n[d].detach(), "dw_ih": getattr(gru, "weight_ih_l0" + sfx).grad,
                    "dw_hh": getattr(gru, "weight_hh_l0" + sfx).grad, "db_ih": getattr(gru, "bias_ih_l0" + sfx).grad,
                    "db_hh": getattr(gru, "bias_hh_l0" + sfx).grad})
    return res, x.grad, (h0.grad if h0.grad is not None else torch.zeros_like(h0))


@pytest.mark.parametrize("T,B,H,ndir,h0,lengths", [
    (5, 9, 12, 2, True, True), (6, 20, 52, 2, False, True), (4, 7, 8, 2, True, False), (3, 5, 64, 1, False, False), (1, 3, 4, 2, True, True),
    (7, 6, 20, 1, True, True)])
def test_restatement_agrees_with_torch_nn_gru_in_float64(T, B, H, ndir, h0, lengths):
    inp = G.inputs(T, B, H, ndir, seed=3, h0=h0, lengths=lengths)
    want, dx, dh0 = _nn_gru(inp)
    got = G.run(inp, torch.float64, fused=True)
    for d in range(ndir):
        for k in ("hs", "h_n"):
            assert float((got[d][k] - want[d][k]).abs().max()) <= 1e-12, (d, k)
    scale = max(float(want[d][k].abs().max()) for d in range(ndir) for k in ("dw_ih", "dw_hh", "db_ih", "db_hh"))
    scale = max(scale, float(dx.abs().max()), float(dh0.abs().max()))
    for d in range(ndir):      # (1e-10 of the largest gradient: an identically zero one has no scale of its own)
        for k in ("dw_ih", "dw_hh", "db_ih", "db_hh"):
            assert float((got[d][k] - want[d][k]).abs().max()) <= 1e-10 * scale, (d, k)
        if h0:
            assert float((got[d]["dh0"] - dh0[d]).abs().max()) <= 1e-10 * scale, d
    assert float((sum(g["dx"] for g in got) - dx).abs().max()) <= 1e-10 * scale


@pytest.mark.parametrize("T,B,H,lengths", [(5, 9, 12, True), (6, 20, 52, False), (34, 4, 64, True), (2, 17, 200, True)])
def test_float32_restatement_agrees_with_the_oracle_direction(T, B, H, lengths):
    inp = G.inputs(T, B, H, 2, seed=5, lengths=lengths)
    got = G.run(inp, torch.float32, fused=True, grad=False)
    for d in range(2):
        hs, h_n = O.gru_direction(inp["x"], inp["w_ih"][d], inp["w_hh"][d], inp["b_ih"][d], inp["b_hh"][d], bool(d), inp["lengths"])
        assert float(G.step_err(got[d]["hs"], hs, "hs").max()) <= 1e-6, d
        assert float(G.step_err(got[d]["h_n"], h_n, "h_n").max()) <= 1e-6, d


@pytest.mark.parametrize("h0,lengths", [(True, True), (False, False)])
def test_dgi_and_dgh_are_the_gradients_the_weight_gradients_are_made_of(h0, lengths):
    """dW_hh = sum dgh_t^T h_prev_t and db_hh = sum dgh_t with h_prev read from hs the way the kernels read it (the step before in
    the direction of travel; the initial state at a row's first live step), against autograd's W_hh / b_hh gradients; a given gi
    (not fused) leaves dgi, dgh unchanged; padded dgi, dgh, hs rows are exactly zero."""
    T, B, H = 6, 11, 20
    inp = G.inputs(T, B, H, 2, seed=9, h0=h0, lengths=lengths)
    res, live = G.run(inp, torch.float64, fused=True), G.valid(inp)
    given = G.run(dict(inp, gi=res_gi(inp)), torch.float64, fused=False)
    for d in range(2):
        r, rev = res[d], inp["reverse"][d]
        start = inp["h0"][d].double() if h0 else torch.zeros(B, H, dtype=torch.float64)
        hprev = torch.zeros(T, B, H, dtype=torch.float64)
        for t in range(T):
            tp = t + 1 if rev else t - 1
            from_hs = (live[tp] if 0 <= tp < T else torch.zeros(B, dtype=torch.bool)).unsqueeze(1)
            hprev[t] = torch.where(from_hs, r["hs"][tp] if 0 <= tp < T else start, start)
        dw = torch.einsum("tbg,tbh->gh", r["dgh"], hprev)
        assert float((dw - r["dw_hh"]).abs().max()) <= 1e-12 * float(r["dw_hh"].abs().max())
        assert float((r["dgh"].sum((0, 1)) - r["db_hh"]).abs().max()) <= 1e-12 * float(r["db_hh"].abs().max())
        for k in ("dgi", "dgh", "hs", "gates"):
            assert float(r[k][~live].abs().max() if bool((~live).any()) else 0.0) == 0.0, k
            assert torch.equal(given[d][k], r[k]), k
        assert torch.equal(r["dgi"][:, :, :2 * H], r["dgh"][:, :, :2 * H])


def res_gi(inp):
    """the float64 projection as a `gi` input: run(fused=False) on it repeats run(fused=True)"""
    T, B, H = inp["T"], inp["B"], inp["H"]
    return torch.stack([(inp["x"].double().reshape(T * B, H) @ inp["w_ih"][d].double().t() + inp["b_ih"][d].double()).reshape(T, B, 3 * H)
                        for d in range(inp["ndir"])])


def test_layout_helpers_round_trip():
    inp = G.inputs(5, 9, 8, 1, seed=2, lengths=True, gathered=True)
    gi, off = inp["gi"][0], G.row_off(inp)
    packed = G.pack(gi, inp)
    assert packed.shape[0] == int(inp["lengths"].sum()) and off[0] == 0 and off[1] == 9
    assert torch.equal(G.unpack(packed, inp), torch.where(G.valid(inp).unsqueeze(2), gi, torch.zeros_like(gi)))
    for pk in (False, True):
        table, index = G.gather_layout(gi, inp, packed=pk)
        assert table.shape[0] <= G.TABLE_ROWS and index.dtype == torch.int64
        assert torch.equal(table[index], packed if pk else gi.reshape(-1, gi.shape[-1]))


def test_check_passes_the_float32_restatement_and_catches_planted_defects():
    """G.check, the assertion of the device test, on a stand-in for a kernel: the float32 restatement passes every array; it does
    not with one 16-unit hidden tile of one late step off by 1e-5, with a row of the ragged last row tile frozen one step early,
    with the reverse direction of one row started at T - 1 instead of length - 1, nor with dgh_n lacking the factor r."""
    case = next(c for c in GS.GRU_F64_CASES if c["id"] == "FAST-5x20x64-shared-h0-lengths")
    ref = G.reference(case)
    inp, T, H = ref["inp"], case["T"], case["H"]
    for d in range(2):
        for k in G.FWD_ARRAYS + G.GRADS:
            assert G.check(f"float32 dir{d}", k, ref["f32"][d][k], ref["f64"][d][k], ref["e32"][d][k])[0], (d, k)
    f32, f64, e32 = ref["f32"][0], ref["f64"][0], ref["e32"][0]
    off = f32["hs"].clone()
    off[T - 2, :, 16:32] *= 1 + 1e-5                                # one 16-unit tile, one late step
    assert not G.check("planted tile", "hs", off, f64["hs"], e32["hs"])[0]
    ln = inp["lengths"]
    row = next(b for b in range(16, 20) if 2 <= int(ln[b]) < T)    # the second row tile has four rows
    last = int(ln[row]) - 1
    hs, h_n = f32["hs"].clone(), f32["h_n"].clone()
    hs[last, row], h_n[row] = 0.0, f32["hs"][last - 1, row]        # frozen (and padded) one step early
    assert not G.check("planted early freeze", "hs", hs, f64["hs"], e32["hs"])[0]
    assert not G.check("planted early freeze", "h_n", h_n, f64["h_n"], e32["h_n"])[0]
    ln2 = ln.clone()
    ln2[row] = T                                                    # the reverse direction of this row starts at T - 1
    late = G.run(dict(inp, lengths=ln2), torch.float32, grad=False)[1]["hs"]
    late = torch.where(G.valid(inp).unsqueeze(2), late, torch.zeros_like(late))
    assert not G.check("planted reverse start", "hs", late, ref["f64"][1]["hs"], ref["e32"][1]["hs"])[0]
    dgh = f32["dgh"].clone()
    dgh[:, :, 2 * H:] = f32["dgi"][:, :, 2 * H:]                    # g_hn = g_n r: the factor left out
    assert not G.check("planted dgh_n", "dgh", dgh, f64["dgh"], e32["dgh"])[0]


@pytest.mark.parametrize("case", GS.GRU_F64_CASES, ids=lambda c: c["id"])
def test_case_meets_the_conditions_of_its_reference(case):
    assert GS.case_route(case, False, cus=256) == case["route"]
    assert (GS.case_route(case, True, cus=256) if case["bwd"] else "") == case["route_bwd"]
    ref = G.reference(case)
    if case.get("packed"):
        ln = ref["inp"]["lengths"]
        assert int(ln[0]) == case["T"] and bool((ln[:-1] >= ln[1:]).all())
    for d, per_dir in enumerate(ref["e32"]):
        for k, e32 in per_dir.items():
            assert bool(torch.isfinite(e32).all()), (d, k)
            worst = float((G.MARGIN * torch.clamp(e32, min=2 * G.U)).max())
            assert worst < G.cap_of(k), f"dir {d} {k}: 8 e32 = {worst:.2e} reaches the cap {G.cap_of(k):.0e}: shorten the case"


def test_cases_meet_every_route_and_variant_in_both_directions():
    fwd, bwd = {c["route"] for c in GS.GRU_F64_CASES}, {c["route_bwd"] for c in GS.GRU_F64_CASES if c["route_bwd"]}
    assert {r.split("*")[0] for r in fwd} == set(GS.ROUTES) and {r.split("*")[0] for r in bwd} == set(GS.ROUTES)
    assert fwd >= {"FAST", "FAST*1", "STREAM", "STREAM*1", "STREAM*2"}
    assert bwd >= {"FAST", "FAST*1", "FAST*2", "FAST*3", "STREAM", "STREAM*1"}
    for c in GS.GRU_F64_CASES:      # an unaligned H = 64 case never names FAST
        assert not (c["H"] == 64 and c.get("unaligned") and "FAST" in (c["route"] + c["route_bwd"])), c["id"]
