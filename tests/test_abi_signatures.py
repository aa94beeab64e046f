"""Every prototype of include/*.h against the signature abi.py and sys.rs give it, without a device.

abi.FAMILIES holds, per header, name -> (restype, argtypes); load_rtmi() applies it.  For every prototype that ends in `;`
this test demands: the function is in exactly one table, its header's; the arity, the class of each argument (pointer, or
a scalar's kind and width) and the return type agree; and wherever sys.rs declares it, arity and pointer class agree there.
The same runs for every RTH_API definition of host/rt_host_c.cpp against load_host()'s table, read through a stub in place
of the library.  The counts are asserted, so a prototype the parser misses cannot pass as success."""
import ctypes as C

import abi_kit as kit
from raytracing_rust_amd import abi

# sys.rs declares nothing of rtmi_session.h (a gap older than this test; adding the bindings is its own change)
NOT_IN_RUST = set(abi.SESSION_SYMBOLS)


def _agree(name, proto, restype, argtypes):
    ret, args = proto
    assert kit.c_class(ret) == kit.ctypes_class(restype), "%s returns %r, the table says %r" % (name, ret, restype)
    assert len(args) == len(argtypes), "%s takes %d arguments, the table lists %d" % (name, len(args), len(argtypes))
    for k, (a, t) in enumerate(zip(args, argtypes)):
        assert kit.c_class(a) == kit.ctypes_class(t), "%s, argument %d: %r against %r" % (name, k, a, t)


def test_every_prototype_agrees_with_its_table_and_with_rust():
    rust, seen, seen_rust = kit.rust_fns(), 0, 0
    for header in kit.HEADERS:
        for name, proto in kit.prototypes(header).items():
            assert [h for h, t in abi.FAMILIES.items() if name in t] == [header], name
            _agree(name, proto, *abi.FAMILIES[header][name])
            seen += 1
            if name in NOT_IN_RUST:
                assert name not in rust
                continue
            rret, rargs = rust[name]
            assert (rret is None) == (proto[0] == "void") and len(rargs) == len(proto[1]), name
            assert [kit.rust_is_pointer(t) for t in rargs] == [kit.c_class(a) == "ptr" for a in proto[1]], name
            assert rret is None or kit.rust_is_pointer(rret) == (kit.c_class(proto[0]) == "ptr"), name
            seen_rust += 1
    assert seen == sum(len(t) for t in abi.FAMILIES.values()) == 110
    for table in abi.FAMILIES.values():
        assert all(isinstance(args, list) for _, args in table.values())  # no function goes without argtypes
    assert seen_rust == len(rust) == 110 - len(NOT_IN_RUST) == 101


class _Recorder:
    """Stands for a loaded library: hands out one attribute bag per function name."""

    def __init__(self, *args, **kwargs):
        self.fns = {}

    def __getattr__(self, name):
        return self.fns.setdefault(name, type("fn", (), {})())


def test_every_host_definition_agrees_with_load_host(monkeypatch):
    monkeypatch.setattr(C, "CDLL", _Recorder)
    monkeypatch.setattr(abi, "_rtmi", None)
    monkeypatch.setattr(abi, "_host", None)
    monkeypatch.setattr(abi._build, "LIBRTMI", __file__)  # any file that exists: nothing is built or loaded
    monkeypatch.setattr(abi._build, "LIBHOST", __file__)
    table = abi.load_host().fns
    defined = kit.host_definitions()
    assert sorted(defined) == sorted(table) and len(defined) == 105
    for name, proto in defined.items():
        _agree(name, proto, table[name].restype, table[name].argtypes)


def test_the_library_exports_the_tables_and_nothing_else():
    """No seam of the implementation shows and no entry is hidden: the rtmi_* names librtmi.so defines are the tables' keys."""
    everything = set().union(*abi.FAMILIES.values())
    assert kit.exported() == everything, sorted(kit.exported() ^ everything)


def test_the_constants_of_every_header_agree():
    """Integer #defines and enumerators: every one abi.py or sys.rs also names has the header's value there."""
    in_abi, in_rust = [], []
    for header in kit.HEADERS:
        a, r = kit.check_constants(header)
        in_abi += a
        in_rust += r
    assert len(in_abi) == 65 and len(in_rust) == 94  # counted from the sources: a parser miss would lower them
