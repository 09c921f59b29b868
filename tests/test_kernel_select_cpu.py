"""Which instantiation of k_bounce a launch takes (no GPU): the library's selector (csrc/pt_api.hip: bounce_form, through the test
library's pt_test_bounce_form) against the chain of ifs it replaced, written out here once more -- that chain is the specification.

A state is nine bits -- the launch's `first` and the renderer's dof, many, sweptCubes, mesh, grouped, tex, bump, plain -- and pt_init
only ever produces states with sweptCubes => many, bump => tex, grouped => many and no mesh and no texture.  A launch's DOF is
first && dof.  The 160 such states reach 48 forms: the 48 kernels the library holds."""
import ctypes as C

STATE = ("first", "dof", "many", "sweptCubes", "mesh", "grouped", "tex", "bump", "plain")      # bit i of state_bits
FORM = ("FIRST", "MANY", "DOF", "MESH", "PLAIN", "CUBES", "GROUPS", "TEX", "BUMP")              # bit i of form_bits


def kb(F, M, D, ME, PL=False, CU=False, GR=False, TX=False, BU=False):
    return sum(int(bool(v)) << i for i, v in enumerate((F, M, D, ME, PL, CU, GR, TX, BU)))


def chain_bump(s, first, dof):
    if s["many"] and s["mesh"]:
        return (kb(1, 1, 1, 1, 0, 1, 0, 1, 1) if dof else kb(1, 1, 0, 1, 0, 1, 0, 1, 1)) if first else kb(0, 1, 0, 1, 0, 1, 0, 1, 1)
    if s["many"]:
        return (kb(1, 1, 1, 0, 0, 1, 0, 1, 1) if dof else kb(1, 1, 0, 0, 0, 1, 0, 1, 1)) if first else kb(0, 1, 0, 0, 0, 1, 0, 1, 1)
    if s["mesh"]:
        return (kb(1, 0, 1, 1, 0, 0, 0, 1, 1) if dof else kb(1, 0, 0, 1, 0, 0, 0, 1, 1)) if first else kb(0, 0, 0, 1, 0, 0, 0, 1, 1)
    return (kb(1, 0, 1, 0, 0, 0, 0, 1, 1) if dof else kb(1, 0, 0, 0, 0, 0, 0, 1, 1)) if first else kb(0, 0, 0, 0, 0, 0, 0, 1, 1)


def chain_tex(s, first, dof):
    if s["bump"]:
        return chain_bump(s, first, dof)
    if s["many"] and s["mesh"]:
        return (kb(1, 1, 1, 1, 0, 1, 0, 1) if dof else kb(1, 1, 0, 1, 0, 1, 0, 1)) if first else kb(0, 1, 0, 1, 0, 1, 0, 1)
    if s["many"]:
        return (kb(1, 1, 1, 0, 0, 1, 0, 1) if dof else kb(1, 1, 0, 0, 0, 1, 0, 1)) if first else kb(0, 1, 0, 0, 0, 1, 0, 1)
    if s["mesh"]:
        return (kb(1, 0, 1, 1, 0, 0, 0, 1) if dof else kb(1, 0, 0, 1, 0, 0, 0, 1)) if first else kb(0, 0, 0, 1, 0, 0, 0, 1)
    return (kb(1, 0, 1, 0, 0, 0, 0, 1) if dof else kb(1, 0, 0, 0, 0, 0, 0, 1)) if first else kb(0, 0, 0, 0, 0, 0, 0, 1)


def chain(s):
    """bounce_kernel(first, first && R().dof) as it stood before the selector: the same ifs, in the same order"""
    first, dof = s["first"], s["first"] and s["dof"]
    if s["tex"]:
        return chain_tex(s, first, dof)
    if s["plain"] and not s["mesh"] and not s["many"] and not dof:
        return kb(1, 0, 0, 0, 1) if first else kb(0, 0, 0, 0, 1)
    if s["grouped"] and not first:
        return kb(0, 1, 0, 0, 0, 1, 1) if s["sweptCubes"] else kb(0, 1, 0, 0, 0, 0, 1)
    if s["grouped"] and not dof:
        return kb(1, 1, 0, 0, 0, 1, 1) if s["sweptCubes"] else kb(1, 1, 0, 0, 0, 0, 1)
    if s["many"] and s["sweptCubes"]:
        if s["mesh"]:
            return (kb(1, 1, 1, 1, 0, 1) if dof else kb(1, 1, 0, 1, 0, 1)) if first else kb(0, 1, 0, 1, 0, 1)
        return (kb(1, 1, 1, 0, 0, 1) if dof else kb(1, 1, 0, 0, 0, 1)) if first else kb(0, 1, 0, 0, 0, 1)
    if s["mesh"] and s["many"]:
        return (kb(1, 1, 1, 1) if dof else kb(1, 1, 0, 1)) if first else kb(0, 1, 0, 1)
    if s["mesh"]:
        return (kb(1, 0, 1, 1) if dof else kb(1, 0, 0, 1)) if first else kb(0, 0, 0, 1)
    if first and dof:
        return kb(1, 1, 1, 0) if s["many"] else kb(1, 0, 1, 0)
    if first:
        return kb(1, 1, 0, 0) if s["many"] else kb(1, 0, 0, 0)
    return kb(0, 1, 0, 0) if s["many"] else kb(0, 0, 0, 0)


def consistent(s):
    return ((not s["sweptCubes"] or s["many"]) and (not s["bump"] or s["tex"]) and
            (not s["grouped"] or (s["many"] and not s["mesh"] and not s["tex"])))


def names(word, table):
    return "|".join(n for i, n in enumerate(table) if (word >> i) & 1) or "0"


def test_the_selector_is_the_chain_it_replaced(pt):
    T = pt.test_lib()
    assert "pt_test_bounce_form" in pt.TEST_ABI_SYMBOLS and not hasattr(pt.lib(), "pt_test_bounce_form")
    assert "pt_test_live_device_buffers" in pt.TEST_ABI_SYMBOLS and not hasattr(pt.lib(), "pt_test_live_device_buffers")
    states = [(bits, {n: bool((bits >> i) & 1) for i, n in enumerate(STATE)}) for bits in range(512)]
    good = [(bits, s) for bits, s in states if consistent(s)]
    assert len(good) == 160
    forms = set()
    for bits, s in good:
        got = C.c_uint32(0xffffffff)
        assert T.pt_test_bounce_form(bits, C.byref(got)) == 0, (names(bits, STATE), T.pt_last_error())
        assert got.value == chain(s), (names(bits, STATE), names(got.value, FORM), names(chain(s), FORM))
        forms.add(got.value)
    assert len(forms) == 48
    # a state pt_init never produces: one of the 48 forms, or an error -- never a form the library does not hold
    for bits, s in states:
        if consistent(s):
            continue
        got = C.c_uint32(0xffffffff)
        rc = T.pt_test_bounce_form(bits, C.byref(got))
        if rc == 0:
            assert got.value in forms, (names(bits, STATE), names(got.value, FORM))
        else:
            assert rc == -1 and got.value == 0xffffffff and b"no k_bounce form" in T.pt_last_error(), names(bits, STATE)   # PT_ERR_INVALID
    # ... and outside the nine bits, or without a result pointer
    assert T.pt_test_bounce_form(512, C.byref(got)) == -1
    assert T.pt_test_bounce_form(0, None) == -1


def test_no_device_buffer_lives_before_the_first_init(pt):
    T = pt.test_lib()
    T.pt_free()                      # (before the first pt_init: a no-op)
    assert T.pt_test_live_device_buffers() == 0
    assert "pt_test_live_handles" in pt.TEST_ABI_SYMBOLS and not hasattr(pt.lib(), "pt_test_live_handles")
    assert T.pt_test_live_handles() == 0
