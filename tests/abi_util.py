"""What the CPU tests of the C ABI share (no device is touched): the header's
text, the four assertions every new entry point gets, and the harness of the
`*_refuse_before_any_launch` tests.  The facts of each entry point - argument
counts, integer positions, every refusal and its code - stay in its test."""
import ctypes
import functools
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "include", "pddp_hip.h")) as _fh:
    HDR = _fh.read()


def assert_entry_points(symbols):
    """Every symbol has a prototype in include/pddp_hip.h, is in the built
    library and in exported_symbols(), and its stem is bound in _SIGS."""
    from pddp_amd import _native
    lib = ctypes.CDLL(_native.LIB_PATH)
    exported = _native.exported_symbols()
    for name in symbols:
        assert re.search(r"\b%s\s*\(" % name, HDR), \
            "%s: no prototype in pddp_hip.h" % name
        assert hasattr(lib, name), "%s: not in %s" % (name, _native.LIB_PATH)
        assert name in exported, "%s: not in exported_symbols()" % name
        assert name[:-4] in _native._SIGS, "%s: not in _SIGS" % name[:-4]


@functools.lru_cache(maxsize=None)
def _cartpole():
    import pddp_amd
    from pddp_amd.examples import cartpole
    enc = pddp_amd.StateEncoding
    model, cost = cartpole.CartpoleDynamicsModel(0.1), cartpole.CartpoleCost()
    return (model.native_problem(enc.IGNORE_UNCERTAINTY, cost),
            model.native_problem(enc.DEFAULT, cost), (ctypes.c_double * 2)())


def cartpole_pointers():
    """(pp, ppd, q): the addresses of a cartpole pddp_problem in the
    IGNORE_UNCERTAINTY and in the DEFAULT encoding, and of a host word that
    stands for every non-null pointer nobody reads.  (The structs live as long
    as the process.)"""
    return tuple(ctypes.addressof(x) for x in _cartpole())


def caller(fn, good):
    """call(*lead, _<i>=value, ...): fn(*lead, *good with argument i replaced,
    stream NULL)."""
    def call(*lead, **change):
        a = list(good)
        for k, v in change.items():
            a[int(k[1:])] = v
        return fn(*lead, *a, None)
    return call
