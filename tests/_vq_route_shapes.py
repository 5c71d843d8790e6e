"""Shapes of the code-assignment dispatch tests (no device): the sweep of the size-query pin (tests/golden/vq_route_sizes.npz) and
VQ_ROUTE_SHAPES -- for every route and variant of g2v_vq_assign_route a shape that selects it and the nearest shapes that miss it.
Every row passes smallm_rows = 1024 explicitly, so the answer does not depend on the bound context.
tests/test_vq_route_host.py holds the table to the query on the CPU; the GPU tests of the quantiser assert through route() that the
kernel a parametrisation means to test is the one its shape selects."""
from gesture2vec_amd import _lib, ops

# (N, E, K) of g2v_vq_assign_bulk_workspace / g2v_vq_assign_bulk_z_workspace, (K, E) of g2v_vq_bx_image_bytes
BULK_NEK = ((131072, 128, 512), (131077, 128, 128), (1 << 20, 128, 512), (4096, 128, 8192), (1, 1, 1), (7, 100, 33), (0, 128, 512))
BULK_Z_NEK = ((32805, 400, 32), (2048, 400, 512), (1 << 20, 400, 400), (20037, 400, 48), (1, 1, 1), (0, 400, 512))
BX_KE = ((128, 128), (256, 128), (384, 128), (512, 128), (640, 128), (33, 100), (0, 128))

ROUTES = {k[len("G2V_VQ_ROUTE_"):]: v for k, v in _lib.CONSTANTS.items() if k.startswith("G2V_VQ_ROUTE_")}
FACTS = {k[len("G2V_VQ_PLAN_"):]: v for k, v in _lib.CONSTANTS.items() if k.startswith("G2V_VQ_PLAN_")}
ROWS = {k[len("G2V_VQ_"):]: v for k, v in _lib.CONSTANTS.items() if k.endswith(("_MIN_ROWS", "_NR2_ROWS", "_NR4_ROWS", "_TILES"))}


def route(form, wants, N, E, K, *, smallm_rows=1024, facts=(), **_):
    """ops.vq_route with the default of the table: "BX", "FUSED*1", "PACKED*2", "PROJECT>SPLIT*8", ...; "" where the call is refused"""
    return ops.vq_route(form, wants, N, E, K, smallm_rows=smallm_rows, facts=facts)


def _row(name, want, form, wants, N, E, K, **kw):
    return dict(name=name, route=want, form=form, wants=wants, N=N, E=E, K=K, **kw)


def _rows(name, want, N, E, K, wants=("FULL", "IDX", "IDX_BULK"), **kw):
    """a ROWS call, and the RAW call that projects and then lands on it, for each of `wants`"""
    out = []
    for w in wants:
        out.append(_row(f"{name}, {w}", want, "ROWS", w, N, E, K, **kw))
        if want and "ENTRY" not in kw.get("facts", ()):
            out.append(_row(f"{name}, {w}, from raw latents", "PROJECT>" + want, "RAW", w, N, E, K, **kw))
    return out


NOT_FULL = ("IDX", "IDX_BULK")
VQ_ROUTE_SHAPES = tuple(
    # ---- RAW, quantized + SSE wanted: the fused kernels of the tuned shapes (E = 128, K % 128 = 0)
    [_row(f"bx, N = {N}, K = {K}", "BX", "RAW", "FULL", N, 128, K) for (N, K) in ((40, 128), (4096, 256), (16, 384), (4096, 512), (1 << 20, 512))]
    + [_row("K = 640: fused, not bx", "FUSED*1", "RAW", "FULL", 4096, 128, 640),
       _row("fused, no room for the image: the codebook in place", "FUSED", "RAW", "FULL", 4096, 128, 1024, facts=("NO_FRAG",)),
       _row("bx keeps its own image", "BX", "RAW", "FULL", 4096, 128, 512, facts=("NO_FRAG",)),
       _row("fused, K = 8192", "FUSED*1", "RAW", "FULL", 40, 128, 8192),
       _row("tuned shape, indices only: never bx", "PROJECT>FAST*1", "RAW", "IDX", 40, 128, 512),
       _row("tuned shape, indices only, bulk accepted, few rows: never bx", "PROJECT>FAST*1", "RAW", "IDX_BULK", 4096, 128, 512),
       _row("tuned shape, misaligned: off the fused kernels", "PROJECT>SPLIT*8", "RAW", "FULL", 40, 128, 512, facts=("UNALIGNED",)),
       _row("K = 64 at E = 128: not a tuned shape", "PROJECT>PACKED*1", "RAW", "FULL", 4096, 128, 64),
       _row("E = 144: not a tuned shape", "PROJECT>PACKED*1", "RAW", "FULL", 4096, 144, 512)]
    # ---- RAW, indices only, bulk accepted: the z-space screen at the checkpoints' width
    + [_row("bulk-z", "BULK_Z", "RAW", "IDX_BULK", 32805, 400, 32),
       _row("bulk-z, first row count", "BULK_Z", "RAW", "IDX_BULK", 32768, 400, 512),
       _row("bulk-z, 2^20 rows, K = 400", "BULK_Z", "RAW", "IDX_BULK", 1 << 20, 400, 400),
       _row("one row below bulk-z", "PROJECT>PACKED*2", "RAW", "IDX_BULK", 32767, 400, 512),
       _row("bulk-z not accepted", "PROJECT>PACKED*4", "RAW", "IDX", 32805, 400, 32),
       _row("bulk-z is indices only", "PROJECT>PACKED*4", "RAW", "FULL", 32805, 400, 512),
       _row("bulk-z, K = 16: below its range", "PROJECT>PACKED*4", "RAW", "IDX_BULK", 32805, 400, 16),
       _row("bulk-z, K = 528: above its range", "PROJECT>PACKED*4", "RAW", "IDX_BULK", 32805, 400, 528),
       _row("bulk-z, K = 40: not whole code tiles", "PROJECT>GENERIC", "RAW", "IDX_BULK", 32805, 400, 40),
       _row("bulk-z, E = 384: another width", "PROJECT>PACKED*4", "RAW", "IDX_BULK", 32805, 384, 512),
       _row("bulk-z, misaligned", "PROJECT>GENERIC", "RAW", "IDX_BULK", 32805, 400, 512, facts=("UNALIGNED",)),
       _row("bulk-z, the projection takes its small-M kernel up to N rows", "PROJECT>PACKED*4", "RAW", "IDX_BULK", 40000, 400, 512, smallm_rows=40000),
       _row("bulk-z, ... one row fewer", "BULK_Z", "RAW", "IDX_BULK", 40000, 400, 512, smallm_rows=39999),
       _row("bulk-z through its entry point: no row count", "BULK_Z", "RAW", "IDX_BULK", 2048, 400, 512, facts=("ENTRY",)),
       _row("bulk-z through its entry point, too few rows", "", "RAW", "IDX_BULK", 2047, 400, 512, facts=("ENTRY",)),
       _row("bulk-z through its entry point, small-M rows", "", "RAW", "IDX_BULK", 4096, 400, 512, smallm_rows=4096, facts=("ENTRY",)),
       _row("bulk-z through its entry point, another width", "", "RAW", "IDX_BULK", 40000, 128, 512, facts=("ENTRY",)),
       _row("bulk-z through its entry point, misaligned", "", "RAW", "IDX_BULK", 40000, 400, 512, facts=("ENTRY", "UNALIGNED"))]
    # ---- ROWS, indices only, bulk accepted: the screen on the projected rows of the tuned shapes
    + [_row("bulk", "BULK*7", "ROWS", "IDX_BULK", 131077, 128, 128),
       _row("bulk, from raw latents", "PROJECT>BULK*9", "RAW", "IDX_BULK", 131072, 128, 512),
       _row("bulk, K = 8192", "BULK*13", "ROWS", "IDX_BULK", 1 << 20, 128, 8192),
       _row("bulk, K = 8320: past its code indices", "RT*4", "ROWS", "IDX_BULK", 1 << 20, 128, 8320),
       _row("one row below bulk", "RT*4", "ROWS", "IDX_BULK", 131071, 128, 512),
       _row("bulk not accepted at 2^20 rows", "RT*4", "ROWS", "IDX", 1 << 20, 128, 512),
       _row("bulk not accepted at 2^20 rows, from raw latents", "PROJECT>RT*4", "RAW", "IDX", 1 << 20, 128, 512),
       _row("bulk is indices only", "RT*4", "ROWS", "FULL", 1 << 20, 128, 512),
       _row("bulk, E = 400", "PACKED*4", "ROWS", "IDX_BULK", 131077, 400, 512),
       _row("bulk, misaligned", "GENERIC", "ROWS", "IDX_BULK", 131077, 128, 512, facts=("UNALIGNED",)),
       _row("bulk through its entry point: no row count", "BULK*9", "ROWS", "IDX_BULK", 64, 128, 512, facts=("ENTRY",)),
       _row("bulk through its entry point, E = 400", "", "ROWS", "IDX_BULK", 131077, 400, 512, facts=("ENTRY",)),
       _row("bulk through its entry point, K = 16384", "", "ROWS", "IDX_BULK", 131077, 128, 16384, facts=("ENTRY",)),
       _row("bulk through its entry point, misaligned", "", "ROWS", "IDX_BULK", 131077, 128, 512, facts=("ENTRY", "UNALIGNED"))]
    # ---- ROWS: the packed kernel and its row tiles per workgroup
    + _rows("packed, first row count", "PACKED*1", 2048, 400, 512)
    + _rows("one row below packed", "GENERIC", 2047, 400, 512)
    + _rows("packed, one row tile, last row count", "PACKED*1", 8191, 48, 64)
    + _rows("packed, two row tiles", "PACKED*2", 8192, 48, 64)
    + _rows("packed, two row tiles, last row count", "PACKED*2", 32767, 400, 400, wants=("FULL", "IDX"))
    + _rows("packed, four row tiles", "PACKED*4", 32768, 400, 400, wants=("FULL", "IDX"))
    + _rows("packed, four row tiles, K below a code tile of the tuned kernels", "PACKED*4", 33000, 128, 48)
    + _rows("packed, E = 608: the widest", "PACKED*1", 4096, 608, 64)
    + _rows("packed_ok is false at E = 640", "GENERIC", 4096, 640, 64)
    + _rows("packed, E = 100: not whole fragments", "GENERIC", 4096, 100, 64)
    + _rows("packed, K = 72: not whole code tiles", "GENERIC", 4096, 400, 72)
    + _rows("packed, no room for the image", "GENERIC", 4096, 400, 512, facts=("NO_FRAG",))
    + _rows("packed, misaligned", "GENERIC", 4096, 400, 512, facts=("UNALIGNED",))
    + _rows("a tuned shape is not packed", "FAST*1", 4096, 128, 512, wants=NOT_FULL)
    + [_row("a tuned shape is not packed, FULL", "FAST*1", "ROWS", "FULL", 4096, 128, 512)]
    + _rows("packed through its entry point: no row count", "PACKED*1", 40, 400, 512, wants=("FULL", "IDX"), facts=("ENTRY",))
    + _rows("packed through its entry point: a tuned shape too", "PACKED*2", 8192, 128, 512, wants=("FULL", "IDX"), facts=("ENTRY",))
    + _rows("packed through its entry point, E = 640", "", 4096, 640, 64, wants=("FULL", "IDX"), facts=("ENTRY",))
    + _rows("packed through its entry point, misaligned", "", 4096, 400, 512, wants=("FULL", "IDX"), facts=("ENTRY", "UNALIGNED"))
    # ---- ROWS: the kernels of the tuned shapes
    # (a RAW call that wants FULL runs these shapes fused, above: no "from raw latents" twin)
    + _rows("fast", "FAST*1", 40, 128, 512, wants=NOT_FULL)
    + _rows("fast, last row count", "FAST*1", 16383, 128, 512, wants=NOT_FULL)
    + _rows("row-tiled, first row count", "RT*4", 16384, 128, 512, wants=NOT_FULL)
    + _rows("row-tiled, a partial last tile", "RT*4", 16389, 128, 512, wants=NOT_FULL)
    + _rows("fast without an image", "FAST*1", 40, 128, 128, wants=NOT_FULL, facts=("NO_FRAG",))
    + [_row(f"{name}, FULL", want, "ROWS", "FULL", N, 128, 512)
       for (name, want, N) in (("fast", "FAST*1", 40), ("fast, last row count", "FAST*1", 16383), ("row-tiled, first row count", "RT*4", 16384))]
    + _rows("E = 128, misaligned: the codes are split", "SPLIT*8", 40, 128, 512, facts=("UNALIGNED",))
    + _rows("E = 128, K = 192: not a tuned shape", "SPLIT*3", 40, 128, 192)
    # ---- ROWS: the generic kernel, the codes split over workgroups while the row tiles are few
    + _rows("split", "SPLIT*8", 40, 100, 512)
    + _rows("split, 64 row tiles", "SPLIT*8", 1024, 100, 512)
    + _rows("65 row tiles: generic", "GENERIC", 1025, 100, 512)
    + _rows("split, 8 code tiles", "SPLIT*2", 40, 100, 128)
    + _rows("7 code tiles: generic", "GENERIC", 40, 100, 112)
    + _rows("split, 13 code tiles over 3 workgroups", "SPLIT*3", 40, 400, 200)
    + _rows("generic", "GENERIC", 40, 32, 48)
    + _rows("generic, one row, one code", "GENERIC", 1, 1, 1)
    + _rows("generic, E = 2544: the widest", "GENERIC", 4096, 2544, 64)
    + _rows("E = 2560: more than 160 KB of LDS", "", 40, 2560, 512)
    + _rows("E = 2545: rounds up to 2560", "", 4096, 2545, 64)
    + _rows("no rows", "", 0, 128, 512)
    + [_row("no rows, from raw latents", "", "RAW", "FULL", 0, 128, 512),
       _row("no codes, from raw latents", "", "RAW", "IDX_BULK", 40000, 400, 0)]
)

# the shapes at which tests/test_gpu_ops.py checks that the Python dispatchers call what the query names: the smallest of each route
DISPATCH_NEK = ((40, 128, 512), (16389, 128, 512), (40, 100, 512), (40, 32, 48), (2048, 400, 512), (8192, 48, 64), (33000, 128, 48),
                (131077, 128, 128), (32805, 400, 32))
