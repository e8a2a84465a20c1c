"""The binding declares the C ABI once (ffmpeg-heaac_amd/prototypes.py, applied in lib()): every function include/*.h
declares has the restype and the argtypes its prototype asks for.  Read in a fresh interpreter, so that nothing another
test did to the shared CDLL can show (no compute calls here)."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA_SYMBOLS = {"heaac_aac_decoder", "ff_sine_windows"}
KINDS = {"int": C.c_int, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double, "long": C.c_long,
         "uint64_t": C.c_uint64}

CHILD = """
import json, sys
sys.path.insert(0, %r)
import __graft_entry__ as g
pkg = g.load_package()
name = lambda t: None if t is None else t.__name__
out = {}
for n in pkg.EXPORTED:
    f = getattr(pkg.lib(), n)
    out[n] = [name(f.restype), None if f.argtypes is None else [name(t) for t in f.argtypes]]
print(json.dumps(out))
"""


def ctype_of(decl, result=False):
    """The ctypes type of one C parameter declaration (or, with `result`, of a return type)."""
    decl = " ".join(decl.split())
    if "*" in decl or "[" in decl:
        return C.c_char_p if result and decl == "const char *" else C.c_void_p
    words = [w for w in decl.split() if w != "const"]
    if not result and len(words) > 1:
        words = words[:-1]                                # the parameter's name
    kind = " ".join(words)
    if result and kind == "void":
        return None
    assert kind in KINDS, "no ctypes type for %r" % decl
    return KINDS[kind]


def declared_prototypes():
    """{name: (restype, [argtypes])} of every function include/*.h declares."""
    protos = {}
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if not h.endswith(".h") or h == "heaac_iso_tables.h":        # (constant tables, no entry points)
            continue
        txt = open(os.path.join(ROOT, "include", h)).read()
        txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
        txt = re.sub(r"//[^\n]*", " ", txt)
        txt = re.sub(r"^\s*#.*$", " ", txt, flags=re.M)
        for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b((?:heaac|ff|av)_\w+)\s*\(([^;{}]*)\)\s*;", txt):
            ret, name, params = m.groups()
            assert name not in protos, name
            params = [] if params.strip() == "void" else params.split(",")
            protos[name] = (ctype_of(ret, result=True), [ctype_of(p) for p in params])
    return protos


def test_every_declared_function_has_its_prototype(pkg):
    protos = declared_prototypes()
    assert set(protos) == set(pkg.EXPORTED) - DATA_SYMBOLS, set(protos) ^ (set(pkg.EXPORTED) - DATA_SYMBOLS)
    out = subprocess.check_output([sys.executable, "-c", CHILD % ROOT], cwd=ROOT)
    bound = json.loads(out.decode().strip().splitlines()[-1])
    name = lambda t: None if t is None else t.__name__
    wrong = []
    for fn, (restype, argtypes) in sorted(protos.items()):
        want = [name(restype), [name(t) for t in argtypes]]
        if bound[fn] != want:
            wrong.append((fn, bound[fn], want))
    assert not wrong, wrong
