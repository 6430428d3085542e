"""CPU-only: the whole ctypes binding of vlatouch/_lib.py against the C headers (tests/abi.py derives C's side): every entry point's
restype and argtypes, every struct's size and every field's offset and size, the multi-tensor table's row as `train.mt_table` writes it,
and every integer code a Python module restates.  The C facts come from one host-only probe built by the compiler the library was built
with; a probe that does not build is a failure (a Python field C lacks, or broken headers), not a skip."""
import ctypes as C
import inspect

import pytest

from tests import abi
from vlatouch import _lib, train


def _show(sig):
    res, args = sig
    return f"({getattr(res, '__name__', res)}, [{', '.join(a.__name__ for a in args)}])"


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if abi.hipcc() is None:
        pytest.skip("no hipcc on this machine")
    try:
        return abi.c_facts(tmp_path_factory.mktemp("abi"))
    except abi.ProbeError as e:
        return e


def _facts(probe):
    if isinstance(probe, abi.ProbeError):
        pytest.fail(str(probe), pytrace=False)
    return probe


def test_signatures_equal_the_header():
    declared = abi.declared_functions()
    assert len(declared) >= 140 and all(n in declared for n in abi.UNBOUND)
    bad = [f"{n}: not in SIGNATURES, the header says {_show(sig)}" for n, sig in declared.items() if n not in abi.UNBOUND and n not in _lib.SIGNATURES]
    bad += [f"{n}: in SIGNATURES but not declared in include/vlatouch.h" for n in _lib.SIGNATURES if n not in declared]
    bad += [f"{n}: SIGNATURES has {_show(sig)}, the header says {_show(declared[n])}" for n, sig in _lib.SIGNATURES.items()
            if n in declared and (sig[0], list(sig[1])) != declared[n]]
    assert not bad, "\n".join(bad)


def test_bound_functions_carry_the_declared_types():
    lib, declared = _lib.lib(), abi.declared_functions()
    bad = []
    for n, want in declared.items():
        if n in abi.UNBOUND:
            continue
        fn = getattr(lib, n)
        if fn.argtypes is None:
            bad.append(f"{n}: no argtypes were set, the header says {_show(want)}")
        elif (fn.restype, list(fn.argtypes)) != want:
            bad.append(f"{n}: bound as {_show((fn.restype, fn.argtypes))}, the header says {_show(want)}")
    assert not bad, "\n".join(bad)


def test_every_structure_of_the_binding_is_checked():
    defined = {c for _, c in inspect.getmembers(_lib, inspect.isclass) if issubclass(c, C.Structure) and c.__module__ == _lib.__name__}
    listed = [c for c, _ in abi.STRUCTS]
    assert len(set(listed)) == len(listed) and len({ct for _, ct in abi.STRUCTS}) == len(listed)
    missing = sorted(c.__name__ for c in defined - set(listed))
    assert not missing, f"ctypes.Structure classes of vlatouch/_lib.py without a row in tests/abi.py STRUCTS: {missing}"
    assert set(listed) <= defined


def test_struct_layouts_equal_c(probe):
    facts, bad = _facts(probe), []
    for cls, ctype in abi.STRUCTS:
        if C.sizeof(cls) != facts["sizeof"][ctype]:
            bad.append(f"sizeof({cls.__name__}) = {C.sizeof(cls)}, sizeof({ctype}) = {facts['sizeof'][ctype]}")
        for name in abi.field_names(cls):
            d = getattr(cls, name)
            if (d.offset, d.size) != facts["fields"][ctype, name]:
                bad.append(f"{cls.__name__}.{name}: (offset, size) = {(d.offset, d.size)}, {ctype}.{name} has {facts['fields'][ctype, name]}")
    assert not bad, "\n".join(bad)


def test_python_fields_account_for_every_byte_of_the_c_struct(probe):
    """C has no field Python lacks, through the sizes: walking the Python fields with C's padding rule (each field at the next multiple
    of its alignment, the struct rounded up to its widest alignment) must land every field on C's offset and end exactly at C's sizeof.
    A C field Python lacks moves a later offset or the size.  (The one thing sizes cannot see is a field that fits an alignment gap.)"""
    facts, bad = _facts(probe), []
    for cls, ctype in abi.STRUCTS:
        end, widest = 0, 1
        for name, ftype in [f[:2] for f in cls._fields_]:
            a = C.alignment(ftype)
            at = -(-end // a) * a
            off, size = facts["fields"][ctype, name]
            if at != off:
                bad.append(f"{cls.__name__}.{name}: the fields before it end at byte {end}, so it belongs at {at}; {ctype}.{name} is at {off}")
            end, widest = off + size, max(widest, a)
        total = -(-end // widest) * widest
        if total != facts["sizeof"][ctype]:
            bad.append(f"{cls.__name__}: its {len(cls._fields_)} fields end at byte {end} ({total} padded); sizeof({ctype}) = {facts['sizeof'][ctype]}: "
                       f"C has fields behind {cls.__name__}.{cls._fields_[-1][0]} that Python lacks")
    assert not bad, "\n".join(bad)


def test_mt_table_writes_the_row_of_MtEntry(probe):
    facts = _facts(probe)
    assert facts["sizeof"]["MtEntry"] == 7 * 8
    assert [facts["fields"]["MtEntry", f] for f in abi.MT_ENTRY] == [(8 * i, 8) for i in range(7)]
    given = dict(p=11, g=12, m=13, v=14, shadow=15, n=16)                                # mt_table's argument order; first_chunk of row 0 is 0
    rows, chunks = train.mt_table([tuple(given.values())])
    assert rows.dtype.itemsize == 8 and tuple(rows.shape) == (1, 7) and rows.is_contiguous() and chunks == 1
    raw = rows.numpy().tobytes()
    assert len(raw) == facts["sizeof"]["MtEntry"]
    for f, want in dict(given, first_chunk=0).items():
        off, size = facts["fields"]["MtEntry", f]
        got = int.from_bytes(raw[off:off + size], "little", signed=True)
        assert got == want, f"train.mt_table puts {got} where MtEntry.{f} (offset {off}) lies; the row was built from {f} = {want}"


def test_constants_equal_c(probe):
    facts = _facts(probe)
    bad = [f"{py} = {val}, {cname} = {facts['constants'][cname]}" for py, val, cname in abi.CONSTANTS if val != facts["constants"][cname]]
    assert not bad, "\n".join(bad)
    assert len(abi.CONSTANTS) >= 60
