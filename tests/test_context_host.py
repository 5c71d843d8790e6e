"""The one route to the library's implementation switches (gesture2vec_amd._lib.Context: set / get / scoped / current) and the
legacy setters it replaced.  Host code only: loading the library and the g2v_ctx_* calls need no GPU."""
import os
import re

import pytest

from gesture2vec_amd import _lib
from gesture2vec_amd._lib import Context, G2VLibraryError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTABLE = [v for k, v in Context.OPTIONS.items() if k != "preclear_notes"]


def _all(ctx):
    return [ctx.get(o) for o in SETTABLE]


@pytest.fixture
def default_untouched():
    """the process's default context reads the same before and after the test"""
    before = _all(Context.current())
    yield before
    assert _all(Context.current()) == before


def test_scoped_restores_exactly_what_set_returned(default_untouched):
    ctx = Context()
    ctx.set(_lib.OPT_PERSISTENT, 3)
    ctx.set(_lib.OPT_GRU_RESIDENT_ROWS, 7)
    both = lambda: (ctx.get(_lib.OPT_PERSISTENT), ctx.get(_lib.OPT_GRU_RESIDENT_ROWS))
    with ctx.scoped(persistent=0, gru_resident_rows=0) as inside:
        assert inside is ctx and both() == (0, 0)
        assert _all(Context.current()) == default_untouched
    assert both() == (3, 7)
    with pytest.raises(ZeroDivisionError):
        with ctx.scoped(persistent=0, gru_resident_rows=0):
            assert both() == (0, 0)
            1 / 0
    assert both() == (3, 7)
    with ctx.scoped(persistent=2):
        with ctx.scoped(persistent=1, gru_resident_rows=5):
            with ctx.scoped(persistent=0):
                assert both() == (0, 5)
            assert both() == (1, 5)
        assert both() == (2, 7)
    assert both() == (3, 7)
    with ctx.scoped():                                        # (nothing to set, nothing to restore)
        assert both() == (3, 7)


def test_argument_checks_change_nothing(default_untouched):
    ctx = Context()
    ctx.set(_lib.OPT_PERSISTENT, 3)
    before = _all(ctx)
    with pytest.raises(TypeError, match="no_such_option"):
        with ctx.scoped(persistent=0, no_such_option=1):
            pytest.fail("entered")
    assert _all(ctx) == before
    with pytest.raises(G2VLibraryError):                      # read-only: the set is refused, what was set before it is put back
        with ctx.scoped(persistent=0, preclear_notes=1):
            pytest.fail("entered")
    assert _all(ctx) == before and ctx.get(_lib.OPT_PRECLEAR_NOTES) == 0
    with pytest.raises(G2VLibraryError, match="99"):
        ctx.set(99, 0)
    with pytest.raises(G2VLibraryError, match="99"):
        ctx.get(99)
    with pytest.raises(G2VLibraryError):
        ctx.set(_lib.OPT_PRECLEAR_NOTES, 0)
    assert _all(ctx) == before


def test_current_follows_the_binding(default_untouched):
    ctx, cur = Context(), Context.current()
    rows = default_untouched[SETTABLE.index(_lib.OPT_SMALLM_ROWS)]
    assert ctx.get(_lib.OPT_SMALLM_ROWS) == rows              # (a new context starts from the defaults)
    with ctx:
        assert cur.set(_lib.OPT_SMALLM_ROWS, rows + 11) == rows
        assert Context.current().get(_lib.OPT_SMALLM_ROWS) == rows + 11
    assert ctx.get(_lib.OPT_SMALLM_ROWS) == rows + 11 and cur.get(_lib.OPT_SMALLM_ROWS) == rows      # landed in ctx, not in the default
    try:
        assert cur.set(_lib.OPT_SMALLM_ROWS, rows + 5) == rows        # outside a binding: the default context
        assert _lib.load().g2v_ctx_get_option(None, _lib.OPT_SMALLM_ROWS) == rows + 5 and ctx.get(_lib.OPT_SMALLM_ROWS) == rows + 11
    finally:
        cur.set(_lib.OPT_SMALLM_ROWS, rows)
    with pytest.raises(G2VLibraryError):                      # a handle on whatever is bound cannot be bound itself
        with cur:
            pytest.fail("entered")
    del cur                                                   # (owns nothing: the default context survives it)
    assert Context.current().get(_lib.OPT_SMALLM_ROWS) == rows


@pytest.mark.parametrize("setter,option,values", [("g2v_linear_set_smallm_rows", "OPT_SMALLM_ROWS", (77, 4096)),
                                                  ("g2v_dec_rollout_set_persistent", "OPT_PERSISTENT", (0, 3)),
                                                  ("g2v_gru_seq_set_cluster", "OPT_GRU_CLUSTER", (0, 1))])
def test_legacy_setters_are_forwards_to_the_bound_context(setter, option, values, default_untouched):
    """The three exported setters of before the contexts are g2v_ctx_set_option(NULL, ...): same previous value, same effect.
    (The only place that still calls them: test_no_stray_calls_of_the_legacy_setters.)"""
    lib, option = _lib.load(), getattr(_lib, option)
    legacy = getattr(lib, setter)
    with Context() as ctx:                                    # (bound: NULL addresses it, the default context stays out of this)
        start = ctx.get(option)
        for v in values:
            a = legacy(v)
            got_a = ctx.get(option)
            ctx.set(option, start)
            b = lib.g2v_ctx_set_option(None, option, v)
            assert a == b == start and ctx.get(option) == got_a == v
            ctx.set(option, start)


def test_no_stray_calls_of_the_legacy_setters():
    pat = re.compile(r"(?:lib|\.load\(\))\.(g2v_dec_rollout_set_persistent|g2v_gru_seq_set_cluster|g2v_linear_set_smallm_rows)\(")
    stray = []
    for top in ("gesture2vec_amd", "scripts", "tests"):
        for d, _, files in os.walk(os.path.join(ROOT, top)):
            for name in files:
                path = os.path.join(d, name)
                if name.endswith((".py", ".sh")) and not os.path.samefile(path, __file__):
                    with open(path, errors="replace") as fh:
                        stray += [f"{os.path.relpath(path, ROOT)}:{n}: {m[1]}" for n, line in enumerate(fh, 1) for m in pat.finditer(line)]
    assert not stray, stray
