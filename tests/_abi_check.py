"""The prototype-against-signature-table check shared by the CPU ABI tests of include/ddpo_hip.h and of the five side headers."""
import ctypes
import re


def check_signatures(header, sigs, count, returns=("int", "size_t")):
    """Every `int|size_t ddpo_*( ... );` prototype of the header file against its row of the ctypes table `sigs`: `count` prototypes and
    rows with the same names, the parameter count, the return type (one of `returns`), a pointer exactly where the binding passes one, and
    the same scalar kind elsewhere — ctypes checks none of this on a positional call."""
    hdr = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    protos = re.findall(r"\b(int|size_t)\s+(ddpo_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr)
    assert len(protos) == len(sigs) == count and {name for _, name, _ in protos} == set(sigs)
    scalars = {"float": ctypes.c_float, "double": ctypes.c_double, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t,
               "uint32_t": ctypes.c_uint32, "int": ctypes.c_int}
    for ret, name, params in protos:
        restype, argtypes = sigs[name]
        params = [] if params.strip() in ("", "void") else [p.strip() for p in params.split(",")]
        assert len(params) == len(argtypes), name
        assert ret in returns, name
        assert (restype is ctypes.c_size_t) == (ret == "size_t") and restype in (ctypes.c_size_t, ctypes.c_int), name
        for i, (p, t) in enumerate(zip(params, argtypes)):
            if "*" in p:
                assert t is ctypes.c_void_p or issubclass(t, ctypes._Pointer), f"{name} argument {i}: {p}"
            else:
                assert t is scalars[p.split()[0]], f"{name} argument {i}: {p}"
