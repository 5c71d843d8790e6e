"""g2v_gru_seq_fwd / _bwd on every route of gru_route_plan (csrc/gru.hip) -- FAST with its four variants, CLUSTER, STEP, RESIDENT and
STREAM with its scalar, vector and two-row-tile bodies -- against the float64 restatement of tests/_gru_ref.py, forward and backward,
at each route's smallest admitting shape and the nearest shapes that exercise an edge of its kernel (GRU_F64_CASES,
tests/_gru_route_shapes.py): an initial state, lengths, packed and gathered gi, a shared (T,B,2H) output buffer, hs_ld % 4 != 0,
the fused projection / dx / weight gradients / quantiser backward, the *_prepared entry points, the scalar body at its LDS limit,
and calls whose arrays start 4 bytes past a 16-byte boundary.  Every output array is compared on its own, per direction and per time
step: e_kernel_t <= min(8 max(e32_t, 2u), cap), all of it from the reference alone.  The backward runs from the device's own saved
arrays.  Each case prints, per array, the worst step's e_kernel, e32, their ratio and the bound.

Two identical calls are compared bit for bit on every route: no route's code has an order that is not fixed (the cluster backward
adds its producers' partial products in ascending order, the fused weight gradients are reduced slab by slab in a fixed order).

Largest figures on the MI355X per route and array, over all cases and directions of the route: e_kernel / max(e32, 2u) (the
quantity the margin of 8 multiplies), then e_kernel and e32 of that step ("unal.": the calls with unaligned arrays; forward arrays
under the forward's route, gradients under the backward's):
          FAST                    FAST*1                  FAST*2                  FAST*3                  CLUSTER
  hs      1.98 2.6e-07 1.3e-07    1.44 2.7e-07 1.9e-07    -                       -                       2.94 4.7e-07 1.6e-07
  h_n     1.85 2.2e-07 1.1e-07    1.40 2.7e-07 1.9e-07    -                       -                       1.80 3.5e-07 2.0e-07
  gates   2.01 3.7e-07 1.8e-07    1.72 4.5e-07 2.6e-07    -                       -                       2.12 4.8e-07 2.3e-07
  dgi     2.66 3.2e-07 1.2e-07    1.82 3.2e-07 1.8e-07    1.65 3.3e-07 2.0e-07    -                       2.58 3.5e-07 1.4e-07
  dgh     2.37 3.0e-07 1.3e-07    1.36 3.2e-07 2.3e-07    -                       -                       2.91 4.7e-07 1.6e-07
  dh0     1.31 2.9e-07 2.2e-07    1.10 2.1e-07 1.9e-07    1.17 1.9e-07 1.7e-07    1.14 1.4e-07 1.1e-07    1.40 1.7e-07 8.7e-08
  dx      -                       1.48 4.3e-07 2.9e-07    1.53 3.5e-07 2.3e-07    1.56 4.2e-07 2.7e-07    -
  dw_hh   -                       -                       1.42 3.1e-07 2.2e-07    1.45 3.7e-07 2.6e-07    -
  db_hh   -                       -                       1.26 2.3e-07 1.8e-07    1.37 2.5e-07 1.8e-07    -
  dw_ih   -                       -                       -                       1.41 3.5e-07 2.5e-07    -
  db_ih   -                       -                       -                       1.73 2.6e-07 1.5e-07    -

          STEP                    RESIDENT                RESIDENT unal.          STREAM                  STREAM unal.
  hs      2.54 5.8e-07 2.3e-07    2.02 3.8e-07 1.9e-07    1.96 3.7e-07 1.9e-07    3.31 6.6e-07 2.0e-07    2.17 5.4e-07 2.5e-07
  h_n     2.54 5.8e-07 2.3e-07    1.86 4.8e-07 2.6e-07    1.62 4.2e-07 2.6e-07    3.19 7.8e-07 2.5e-07    2.17 5.4e-07 2.5e-07
  gates   2.17 6.0e-07 2.7e-07    2.56 7.0e-07 2.7e-07    2.27 6.5e-07 2.9e-07    4.73 1.4e-06 3.1e-07    2.21 6.2e-07 2.8e-07
  dgi     2.09 2.6e-07 1.2e-07    2.22 2.7e-07 1.2e-07    -                       2.81 4.5e-07 1.6e-07    2.77 4.1e-07 1.5e-07
  dgh     1.83 2.5e-07 1.4e-07    2.02 3.4e-07 1.7e-07    -                       3.12 4.8e-07 1.5e-07    3.58 4.9e-07 1.4e-07
  dh0     2.08 3.4e-07 1.6e-07    1.77 3.0e-07 1.7e-07    -                       2.57 3.6e-07 1.4e-07    2.00 2.6e-07 1.3e-07

          STREAM*1                STREAM*1 unal.          STREAM*2
  hs      2.25 5.0e-07 2.2e-07    1.72 3.8e-07 2.2e-07    2.16 3.4e-07 1.6e-07
  h_n     2.25 5.0e-07 2.2e-07    1.44 2.3e-07 1.6e-07    2.00 3.5e-07 1.7e-07
  gates   1.95 5.7e-07 2.9e-07    2.34 6.8e-07 2.9e-07    1.66 5.2e-07 3.1e-07
  dgi     2.10 2.8e-07 1.3e-07    2.59 4.0e-07 1.6e-07    -
  dgh     2.19 3.3e-07 1.5e-07    2.48 4.0e-07 1.6e-07    -
  dh0     1.63 2.5e-07 1.5e-07    1.61 3.0e-07 1.9e-07    -

Largest ratio: 4.73 (gates of STREAM-2x16x1264-most-lds, direction 0, step 1; hs and h_n of the same case 3.3 and 3.2).  That is the
scalar body at its LDS limit: gh is a contraction over 1264 terms, which the kernel adds in one MFMA chain of 316 k-steps while the
float32 restatement's matrix product adds it in blocks -- the kernel's error grows with the chain, e32 does not.  Every other route
and array stays at or below 3.6; the unaligned calls sit where the aligned ones of their route sit.

What was settled from the code before any unaligned case ran: the FAST kernels move gi, b_hh, hs, h_n, gates, x, b_ih (forward) and
gates, dgi, dgh, hs, h0, dh0, d_hs, d_hn, dx, wslab (backward) as float4s, and the plan took FAST on H == 64 and the leading
dimensions alone.  The plan now asks for their alignment (include/g2v.h), an H == 64 call that lacks it runs on
the next route (the three -unaligned and -split-unaligned cases at the end of the list), and the fused fields, which only FAST serves,
are refused (the last test of this file).  Every route reads its workspace region as 16-byte vectors -- FAST, RESIDENT and STREAM
their fragment packs -- which no alignment list covered outside STEP's: an unaligned workspace is now G2V_ERR_ARG.
"""
import ctypes as C

import pytest
import torch

import _gru_ref as G
from _dev_arrays import DEV, Arrays
from _gru_route_shapes import GRU_F64_CASES, case_facts

pytestmark = pytest.mark.gpu
NAN = float("nan")
SPLIT_ONLY = ("w_hh", "h_n", "d_hn")      # on STEP's list, on no vector body's list in either direction of travel (h0 is on the backward's)
# the plan's alignment lists (include/g2v.h at g2v_gru_seq_route), by direction of travel: fact -> the fields it covers
LISTS = ({"SPLIT_UNALIGNED": ("gi", "w_hh", "b_hh", "h0", "gates", "h_n"), "VEC_UNALIGNED": ("gi", "b_hh", "hs", "gates"),
          "FAST_UNALIGNED": ("x", "b_ih")},
         {"SPLIT_UNALIGNED": ("gates", "dgi", "dgh", "d_hn", "h0", "dh0"), "VEC_UNALIGNED": ("gates", "dgi", "dgh", "hs", "h0", "dh0", "d_hs"),
          "D_HN_UNALIGNED": ("d_hn",), "FAST_UNALIGNED": ("dx", "wslab")})


@pytest.fixture(scope="module")
def ops():
    from gesture2vec_amd import _lib, ops as o
    assert _lib.load().g2v_device_ok() == 1, "no gfx950 device visible"
    return o


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else t.dtype)


def _same(a, b):
    if a is None or b is None:
        return a is b
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _alloc(case):
    """name -> Arrays: which arrays of this case's calls start 4 bytes past a 16-byte boundary"""
    ua, al, un = case.get("unaligned"), Arrays(False), Arrays(True)
    names = SPLIT_ONLY if ua == "split" else ("d_hn",) if ua == "d_hn" else ua if isinstance(ua, tuple) else ()
    return lambda name: un if ua == "all" or name in names else al


def _unaligned_facts(arr, ndir, backward):
    """the G2V_GRU_PLAN_*_UNALIGNED facts of a call, from the pointers it passes (NULL counts as aligned)"""
    return {fact for fact, fields in LISTS[backward].items() if any((getattr(arr[d], f) or 0) % 16 for d in range(ndir) for f in fields)}


def _declared(case, backward):
    return {f for f in case_facts(case, backward) if f.endswith("_UNALIGNED")}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _workspace(nbytes):
    ws = torch.zeros(max(int(nbytes), 16), dtype=torch.uint8, device=DEV)
    assert ws.data_ptr() % 16 == 0
    return ws


def _ld(case, key):
    return case.get(key) or (2 * case["H"] if case.get("shared") else case["H"])


def _rows(A, name, case, ld, fill):
    """the (T,B,H) views of `ndir` arrays with row stride ld: halves of one (T,B,2H) buffer, or each inside its own (T,B,ld) one"""
    T, B, H, ndir = case["T"], case["B"], case["H"], case["ndir"]
    if case.get("shared"):
        buf = A(name).full((T, B, 2 * H), fill)
        return [buf[:, :, d * H:(d + 1) * H] for d in range(ndir)], [buf]
    bufs = [A(name).full((T, B, ld), fill) for _ in range(ndir)]
    return [b[:, :, :H] for b in bufs], bufs


def _forward(ops, lib, case, inp, dev=None, ws=None, prepared=False, want_rc=0):
    """one g2v_gru_seq_fwd call into NaN-filled outputs -> (per-direction dicts of device tensors, shared inputs)"""
    from gesture2vec_amd import _lib
    T, B, H, ndir, A = case["T"], case["B"], case["H"], case["ndir"], _alloc(case)
    hs_ld = _ld(case, "hs_ld")
    if dev is None:      # the inputs, placed once per case: a second call reads the same arrays
        dev = {"lengths": A("lengths").put(inp["lengths"]) if inp["lengths"] is not None else None,
               "x": A("x").put(inp["x"]) if case.get("fused") else None, "dirs": []}
        for d in range(ndir):
            e = {"w_hh": A("w_hh").put(inp["w_hh"][d]), "b_hh": A("b_hh").put(inp["b_hh"][d]),
                 "h0": A("h0").put(inp["h0"][d]) if inp["h0"] is not None else None}
            if case.get("fused"):
                e.update(w_ih=A("w_ih").put(inp["w_ih"][d]), b_ih=A("b_ih").put(inp["b_ih"][d]))
            elif case.get("gathered"):
                table, index = G.gather_layout(inp["gi"][d], inp, packed=bool(case.get("packed")))
                e.update(gi=A("gi").put(table), gi_gather=A("gi_gather").put(index))
            else:
                e["gi"] = A("gi").put(G.pack(inp["gi"][d], inp) if case.get("packed") else inp["gi"][d])
            dev["dirs"].append(e)
    hs, hs_bufs = _rows(A, "hs", case, hs_ld, NAN)
    out = [{"hs": hs[d], "h_n": A("h_n").full((B, H), NAN), "gates": A("gates").full((T, B, 4 * H), NAN)} for d in range(ndir)]
    arr = (_lib.GruDir * ndir)()
    ro = ops._row_off_array(G.row_off(inp), T) if case.get("packed") else None
    for d in range(ndir):
        e = dev["dirs"][d]
        for name in ("gi", "w_hh", "b_hh", "h0", "w_ih", "b_ih", "gi_gather"):
            setattr(arr[d], name, ops._p(e.get(name)))
        arr[d].x = ops._p(dev["x"])
        for name in ("hs", "h_n", "gates"):
            setattr(arr[d], name, ops._p(out[d][name]))
        arr[d].reverse, arr[d].in_dim = int(inp["reverse"][d]), H if case.get("fused") else 0
        if ro is not None:
            arr[d].gi_row_off = ro
    ws = ws if ws is not None else _workspace(lib.g2v_gru_seq_fwd_workspace(ndir, H))
    fn = lib.g2v_gru_seq_fwd_prepared if prepared else lib.g2v_gru_seq_fwd
    rc = fn(arr, ndir, ops._p(dev["lengths"]), hs_ld, T, B, H, ws.data_ptr(), ws.numel(), _stream())
    torch.cuda.synchronize()
    assert rc == want_rc, (rc, lib.g2v_last_error())
    dev["hs_bufs"], dev["unaligned"] = hs_bufs, _unaligned_facts(arr, ndir, False)
    return out, dev


def _backward(ops, lib, case, inp, dev, saved, bdev=None, ws=None, prepared=False, want_rc=0):
    """one g2v_gru_seq_bwd call from the device's own hs / gates into NaN-filled outputs"""
    from gesture2vec_amd import _lib
    T, B, H, ndir, A = case["T"], case["B"], case["H"], case["ndir"], _alloc(case)
    G3, wgrad, packed = 3 * H, case.get("wgrad", 0), bool(case.get("packed"))
    if bdev is None:
        d_hs, _ = _rows(A, "d_hs", case, _ld(case, "d_hs_ld"), 0.0)
        for d in range(ndir):
            d_hs[d].copy_(inp["d_hs"][d])
        bdev = {"d_hs": d_hs, "d_hn": [A("d_hn").put(inp["d_hn"][d]) for d in range(ndir)],
                "x": dev["x"] if dev["x"] is not None else (A("x").put(inp["x"]) if wgrad == 2 else None),
                "hn_z": [Arrays(False).put(inp["hn_z"][d]) for d in range(ndir)] if case.get("hn") else None,
                "hn_q": [Arrays(False).put(inp["hn_q"][d]) for d in range(ndir)] if case.get("hn") else None,
                "hn_gloss": torch.tensor([G.HN_GLOSS], device=DEV) if case.get("hn") else None}
    nrows = int(inp["lengths"].sum()) if packed else T * B
    out = []
    for d in range(ndir):
        o = {"dgi": None if case.get("no_dgi") else A("dgi").full((nrows, G3) if packed else (T, B, G3), NAN),
             "dgh": None if case.get("no_dgi") else A("dgh").full((T, B, G3), NAN), "dh0": A("dh0").full((B, H), NAN)}
        if case.get("fused"):
            o["dx"] = A("dx").full((T, B, H), NAN)
        if wgrad:
            o.update(dw_hh=A("dw_hh").full((G3, H), NAN), db_hh=A("db_hh").full((G3,), NAN),
                     wslab=A("wslab").full((int(lib.g2v_gru_seq_bwd_wslab_bytes(B, H)) // 4,), 0.0))
        if wgrad == 2:
            o.update(dw_ih=A("dw_ih").full((G3, H), NAN), db_ih=A("db_ih").full((G3,), NAN))
        out.append(o)
    arr = (_lib.GruDirBwd * ndir)()
    ro = ops._row_off_array(G.row_off(inp), T) if packed else None
    for d in range(ndir):
        e, o = dev["dirs"][d], out[d]
        fields = dict(d_hs=bdev["d_hs"][d], d_hn=bdev["d_hn"][d], hs=saved[d]["hs"], h0=e["h0"], gates=saved[d]["gates"], w_hh=e["w_hh"],
                      dgi=o["dgi"], dgh=o["dgh"], dh0=o["dh0"], w_ih=e.get("w_ih") if case.get("fused") else None, dx=o.get("dx"),
                      x=bdev["x"] if wgrad == 2 else None, dw_hh=o.get("dw_hh"), db_hh=o.get("db_hh"), dw_ih=o.get("dw_ih"),
                      db_ih=o.get("db_ih"), wslab=o.get("wslab"))
        if case.get("hn"):
            fields.update(hn_z=bdev["hn_z"][d], hn_q=bdev["hn_q"][d], hn_gloss=bdev["hn_gloss"])
            arr[d].hn_coef = G.HN_COEF
        for name, t in fields.items():
            setattr(arr[d], name, ops._p(t))
        arr[d].reverse, arr[d].in_dim = int(inp["reverse"][d]), H if case.get("fused") else 0
        if ro is not None:
            arr[d].dgi_row_off = ro
    ws = ws if ws is not None else _workspace(lib.g2v_gru_seq_bwd_workspace(ndir, H))
    fn = lib.g2v_gru_seq_bwd_prepared if prepared else lib.g2v_gru_seq_bwd
    rc = fn(arr, ndir, ops._p(dev["lengths"]), _ld(case, "d_hs_ld"), _ld(case, "hs_ld"), T, B, H, ws.data_ptr(), ws.numel(), _stream())
    torch.cuda.synchronize()
    assert rc == want_rc, (rc, lib.g2v_last_error())
    bdev["unaligned"] = _unaligned_facts(arr, ndir, True)
    return out, bdev


@pytest.mark.parametrize("case", GRU_F64_CASES, ids=lambda c: c["id"])
def test_gru_seq_matches_float64_on_its_route(ops, case):
    from gesture2vec_amd import _lib
    lib = _lib.load()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus != 256:
        pytest.skip(f"GRU_F64_CASES names the routes of a device with 256 CUs; this one has {cus}")
    T, B, H, ndir = case["T"], case["B"], case["H"], case["ndir"]
    ref = G.reference(case)
    inp, live, packed = ref["inp"], G.valid(ref["inp"]), bool(case.get("packed"))
    bad = []

    def held(d, name, got, **kw):
        got, want = G.defined(name, got.cpu(), inp, **kw), G.defined(name, ref["f64"][d][name], inp, **kw)
        assert not torch.isnan(got).any(), f"dir {d} {name}: part of what the header defines was left unwritten"
        ok, line, *_ = G.check(f"{case['id']} dir{d}", name, got, want, ref["e32"][d][name])
        if not ok:
            bad.append(line)

    def no_fault(when):
        if "CLUSTER" in (case["route"], case["route_bwd"]):
            assert lib.g2v_dec_rollout_persist_fault(0) == 0, f"a bounded wait ran out ({when})"

    options = dict(gru_cluster=case.get("cluster", 1), gru_resident_rows=case.get("resident_rows", 1025),
                   gru_resident_bwd=case.get("resident_bwd", 1))
    with _lib.Context.current().scoped(**options):
        assert ops.gru_route(T, B, H, ndir, facts=case_facts(case, False)) == case["route"]
        if case["bwd"]:
            assert ops.gru_route(T, B, H, ndir, backward=True, facts=case_facts(case, True)) == case["route_bwd"]
        # ---------------------------------------------------------------------------------------------------------- forward
        no_fault("before the forward")
        saved, dev = _forward(ops, lib, case, inp)
        no_fault("forward")
        assert dev["unaligned"] == _declared(case, False), "the facts the route was asked with are not those of the pointers passed"
        for d in range(ndir):
            for name in G.FWD_ARRAYS:
                held(d, name, saved[d][name])
            assert not bool((_bits(saved[d]["hs"].cpu())[~live] != 0).any()), f"dir {d}: padded hs is not bitwise zero"
        for buf in dev["hs_bufs"]:      # hs_ld > H on a buffer of its own: the columns past H belong to the caller
            if buf.shape[2] != H and not case.get("shared"):
                assert bool(torch.isnan(buf[:, :, H:]).all()), "hs: columns past H were written"
        assert not bad, "\n".join(bad)
        saved2, _ = _forward(ops, lib, case, inp, dev)
        no_fault("second forward")
        for d in range(ndir):
            for name in G.FWD_ARRAYS:
                assert _same(saved[d][name], saved2[d][name]), f"two forwards differ: dir {d} {name}"
        if case.get("prepared"):      # g2v_gru_seq_prepare + the *_prepared entry points: bitwise the plain call
            ws_f, ws_b = _workspace(lib.g2v_gru_seq_fwd_workspace(ndir, H)), _workspace(lib.g2v_gru_seq_bwd_workspace(ndir, H))
            whh = (C.c_void_p * ndir)(*[e["w_hh"].data_ptr() for e in dev["dirs"]])
            rc = lib.g2v_gru_seq_prepare(whh, None, ndir, H, 0, ws_f.data_ptr(), ws_f.numel(), ws_b.data_ptr(), ws_b.numel(), _stream())
            assert rc == 0, lib.g2v_last_error()
            saved3, _ = _forward(ops, lib, case, inp, dev, ws=ws_f, prepared=True)
            for d in range(ndir):
                for name in G.FWD_ARRAYS:
                    assert _same(saved[d][name], saved3[d][name]), f"the prepared forward differs: dir {d} {name}"
        if not case["bwd"]:
            return
        # --------------------------------------------------------------------------------------------------------- backward
        grads, bdev = _backward(ops, lib, case, inp, dev, saved)
        no_fault("backward")
        assert bdev["unaligned"] == _declared(case, True), "the facts the route was asked with are not those of the pointers passed"
        wgrad = case.get("wgrad", 0)
        names = ["dh0"] + (["dx"] if case.get("fused") else []) + (["dw_hh", "db_hh"] if wgrad else []) + (["dw_ih", "db_ih"] if wgrad == 2 else [])
        for d in range(ndir):
            g = grads[d]
            if not case.get("no_dgi"):
                if wgrad < 2:
                    dgi = G.unpack(g["dgi"].cpu(), inp) if packed else g["dgi"]
                    assert not torch.isnan(g["dgi"]).any(), f"dir {d} dgi: a row inside its sequence was left unwritten"
                    held(d, "dgi", dgi, packed=packed)
                else:
                    assert bool(torch.isnan(g["dgi"]).all()), f"dir {d}: dgi is not written once dw_ih is fused"
                if wgrad < 1:
                    held(d, "dgh", g["dgh"])
                    assert not bool((_bits(g["dgh"].cpu())[~live] != 0).any()), f"dir {d}: padded dgh is not bitwise zero"
                else:
                    assert bool(torch.isnan(g["dgh"]).all()), f"dir {d}: dgh is not written once dw_hh is fused"
            for name in names:
                held(d, name, g[name])
        assert not bad, "\n".join(bad)
        grads2, _ = _backward(ops, lib, case, inp, dev, saved2, bdev)
        no_fault("second backward")
        for d in range(ndir):
            for name in ["dgi", "dgh"] + names:
                assert _same(grads[d][name], grads2[d][name]), f"two backwards differ: dir {d} {name}"
        if case.get("prepared"):
            grads3, _ = _backward(ops, lib, case, inp, dev, saved, bdev, ws=ws_b, prepared=True)
            for d in range(ndir):
                for name in ["dgi", "dgh"] + names:
                    assert _same(grads[d][name], grads3[d][name]), f"the prepared backward differs: dir {d} {name}"


# ---- H = 64 with one array 4 bytes past a 16-byte boundary: the call leaves FAST, and what only FAST serves is refused -------------
_FUSED = next(c for c in GRU_F64_CASES if c["id"] == "FAST*1-5x37x64-wgrad-hh-ih")
FWD_LIST = ("x", "b_ih", "b_hh", "hs", "h_n", "gates", "w_hh", "h0")
BWD_LIST = ("d_hs", "d_hn", "dgi", "dgh", "dh0", "dx", "wslab")
BWD_SAVED = ("hs", "gates", "h0", "x")      # what the backward reads of the forward's: moved to an unaligned copy


def _untouched(outs, skip=("wslab",)):
    return all(bool(torch.isnan(t).all()) for o in outs for k, t in o.items() if t is not None and k not in skip)


@pytest.mark.parametrize("name", FWD_LIST + BWD_LIST + ("workspace",))
def test_fused_h64_call_with_one_array_unaligned_is_refused_before_anything_is_launched(ops, name):
    """The fused projection / dx / weight gradients exist on FAST alone, and FAST moves every array as float4s: with any one of them
    only 4-byte aligned the plan leaves FAST (a call without the fused fields then runs on the next route: the unaligned cases
    above) and the fused call is G2V_ERR_UNSUPPORTED with every output as it was.  x of the fused dW_ih is not on a list: it makes
    the weight-gradient group incomplete, G2V_ERR_ARG.  A workspace that is not 16-byte aligned is G2V_ERR_ARG on every route."""
    from gesture2vec_amd import _lib
    lib = _lib.load()
    case, ref = _FUSED, G.reference(_FUSED)
    inp, ndir, H = ref["inp"], _FUSED["ndir"], _FUSED["H"]
    odd = dict(case, unaligned=(name,))
    rc = _lib.ERR_ARG if name == "workspace" else _lib.ERR_UNSUPPORTED
    off_ws = lambda nbytes: _workspace(nbytes + 16)[4:]
    if name in FWD_LIST + ("workspace",):
        outs, _ = _forward(ops, lib, odd, inp, want_rc=rc, ws=off_ws(lib.g2v_gru_seq_fwd_workspace(ndir, H)) if name == "workspace" else None)
        assert (b"16-byte aligned" if name == "workspace" else b"fused input projection") in lib.g2v_last_error()
        assert _untouched(outs), "a refused forward wrote an output"
    if name in BWD_LIST + BWD_SAVED + ("workspace",):
        saved, dev = _forward(ops, lib, case, inp)
        un = Arrays(True)
        if name in ("hs", "gates"):
            saved = [dict(s, **{name: un.put(s[name])}) for s in saved]
        elif name == "h0":
            dev = dict(dev, dirs=[dict(e, h0=un.put(e["h0"])) for e in dev["dirs"]])
        elif name == "x":
            dev, rc = dict(dev, x=un.put(dev["x"])), _lib.ERR_ARG
        grads, bdev = _backward(ops, lib, odd, inp, dev, saved, want_rc=rc,
                                ws=off_ws(lib.g2v_gru_seq_bwd_workspace(ndir, H)) if name == "workspace" else None)
        assert bdev["unaligned"] == ({f for f, fields in LISTS[1].items() if name in fields})
        assert (b"16-byte aligned" if name == "workspace" else b"fused weight gradients" if name == "x" else b"fused input gradient") in lib.g2v_last_error()
        assert _untouched(grads), "a refused backward wrote an output"
