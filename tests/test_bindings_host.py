"""CPU-only: the table of _lib that the ctypes bindings of the features next to the sweep are made from (_lib.FEATURES).  Every row's C
symbols exist and are declared with the row's parameter block, its callables exist under the names the table spells; a refused call
raises the text of its own feature's buffer, walked over all rows with two refusals in turn so that neighbours leave different texts;
and the one helper that turns a return code into an exception."""
import ctypes

import numpy as np
import pytest

import mcq_amd

abi = mcq_amd.abi
_lib = mcq_amd._lib
quench, heatbath, tempering = mcq_amd.quench, mcq_amd.heatbath, mcq_amd.tempering

ROWS = tuple(_lib.FEATURES.items())


def test_the_table_names_every_feature():
    assert tuple(_lib.FEATURES) == ("population", "quench", "quench_pairs", "hop", "hop3d", "tabu", "tabu3d", "relink", "quench3d", "heatbath",
                                    "heatbath3d", "temper", "temper3d")
    assert {f: r.entries[2:] for f, r in ROWS if len(r.entries) > 2} == {"heatbath": ("heatbath_counters_device",), "temper": ("temper_counters_device",)}


@pytest.mark.parametrize("feature,row", ROWS, ids=[f for f, _ in ROWS])
def test_symbols_declarations_and_callables(feature, row):
    L = _lib.lib()
    last = getattr(L, f"mcq_{row.prefix}_last_error")
    assert last.restype is ctypes.c_char_p and isinstance(last(), bytes)
    assert issubclass(row.struct, ctypes.Structure) and getattr(abi, row.struct.__name__) is row.struct
    if feature == "population":  # its calls are written out in lib(): mcq_resample_*
        assert row.entries == () and L.mcq_resample_plan_host.argtypes[0] is ctypes.POINTER(row.struct)
        return
    assert row.entries[:2] == (feature + "_host", feature + "_device")
    for name in row.entries:
        fn = getattr(L, "mcq_" + name)  # AttributeError for a symbol the library does not export
        host = name.endswith("_host")
        assert fn.restype is ctypes.c_int and fn.argtypes[0] is ctypes.POINTER(row.struct), name
        assert list(fn.argtypes[1:]) == ([] if host else [ctypes.c_void_p]), name
        call = getattr(_lib, name)
        assert callable(call) and call.__name__ == name and "mcq_" + name in call.__doc__ and "abi." + row.struct.__name__ in call.__doc__
        assert call.__code__.co_varnames[: call.__code__.co_argcount] == (("q",) if host else ("q", "stream"))
        assert (fn(None) if host else fn(None, None)) == abi.EINVAL and b"NULL" in last()  # refused by host code: nothing is launched


def _refused_block(feature, which):
    """A parameter block that the feature refuses, from its wrapper's own builder: no chain at a valid N (which = 0) or N = 1 (which = 1).
    (Each of the 12 features refuses either with MCQ_EINVAL before it reads a pointer.)"""
    N, n = ((6, 0), (1, 4))[which]
    tab = abi.heatbath_table([])
    return {
        "quench": lambda: quench._block(N, n, 0),
        "quench_pairs": lambda: quench._block_pairs(N, n, 0),
        "hop": lambda: quench._block_hop(N, n, 1, 2, 0, "pairs", 0),
        "hop3d": lambda: quench._block_hop3d(N, N * N, n, 1, 2, 0, 0),
        "tabu": lambda: quench._block_tabu(N, n, 1, 10, 0, 0, 0),
        "tabu3d": lambda: quench._block_tabu3d(N, N * N, n, 1, 10, 0, 0, 0),
        "relink": lambda: quench._block_relink(N, n, 0, 1, "pairs", 0),
        "quench3d": lambda: quench._block3d(N, N * N, n, 0),
        "heatbath": lambda: heatbath._block(N, n, 0, 0, tab),
        "heatbath3d": lambda: heatbath._block3d(N, N * N, n, 0, 0, tab),
        "temper": lambda: tempering._block(N, n, 0, 0, 4, 1, 1, 1),
        "temper3d": lambda: tempering._block3d(N, N * N, n, 0, 0, 4, 1, 1, 1),
    }[feature]()


def test_a_refusal_is_read_from_the_features_own_buffer():
    L = _lib.lib()
    before = None
    for i, (feature, row) in enumerate(ROWS):
        with pytest.raises(ValueError) as e:
            if feature == "population":  # population = 0 is the first thing its validator reports
                _lib.resample_plan_host(np.zeros(16, dtype=np.int32), 0, np.ones(4, dtype=np.uint32), np.zeros(1, dtype=np.uint32))
            else:
                getattr(_lib, feature + "_host")(_refused_block(feature, i % 2))
        text = str(e.value)
        assert text and text == getattr(L, f"mcq_{row.prefix}_last_error")().decode(), feature
        assert ("population" if feature == "population" else "N out of range" if i % 2 else "n_chains") in text, (feature, text)
        assert text != before, (feature, text)
        before = text
    # every buffer still holds its own text: a later feature's refusal did not go through an earlier one's
    texts = [getattr(L, f"mcq_{row.prefix}_last_error")().decode() for _, row in ROWS]
    assert all(a != b for a, b in zip(texts, texts[1:]))


def test_return_codes_become_exceptions():
    calls = []

    def last_error():
        calls.append(1)
        return b"the text \xff of the stub"

    assert _lib._raise(abi.OK, last_error) is None and not calls  # nothing is read behind a call that went through
    for rc, exc in ((abi.EINVAL, ValueError), (abi.ENOMEM, MemoryError), (-77, _lib.McqError)):
        with pytest.raises(exc) as e:
            _lib._raise(rc, last_error)
        assert type(e.value) is exc and str(e.value) == "the text � of the stub"  # decoded with errors="replace"
    assert issubclass(_lib.McqError, RuntimeError) and len({abi.OK, abi.EINVAL, abi.ENOMEM, -77}) == 4
    # the sweep's own check and population annealing's read their own buffers through the same helper
    p = abi.make_params(8, 10, "random", {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}, 4, mcmc_type="board")
    p.N = 1
    with pytest.raises(ValueError) as e:
        _lib.sweep_variant(p)
    assert str(e.value) == _lib.lib().mcq_last_error().decode() != ""
    with pytest.raises(ValueError) as e2:
        _lib._check(abi.EINVAL)
    assert str(e2.value) == str(e.value)
    with pytest.raises(ValueError, match="table_len"):
        _lib.resample_plan_host(np.zeros(16, dtype=np.int32), 16, np.zeros(0, dtype=np.uint32), np.zeros(1, dtype=np.uint32))
    with pytest.raises(ValueError) as e:
        _lib._check_population(abi.EINVAL)
    assert "table_len" in str(e.value)
