"""The ctypes side of include/ptv2_hip.h, derived from the header's text at import.

The header is the contract and is written in a small, regular subset of C: `#define NAME integer`, anonymous enums,
`typedef struct NAME {...} NAME;` and prototypes.  `parse()` reads exactly that and raises on anything else, so a
constant, a struct layout or a launcher signature is written once, in the header:

    consts      {name: int}                    every integer #define and enumerator
    structs     {name: ctypes.Structure}       field for field, in header order
    signatures  {name: (restype, argtypes)}    every prototype

Pointers are c_void_p (callers pass tensor.data_ptr() / ctypes.addressof()), except `char *`, which is c_char_p.
"""
import ctypes
import os
import re

HEADER = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ptv2_hip.h"))

_VALUES = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "float": ctypes.c_float, "double": ctypes.c_double,
           "long long": ctypes.c_longlong, "size_t": ctypes.c_size_t}
_POINTEES = ("void", "char", "unsigned long long")  # known behind a star only
_TYPE = re.compile(r"\s*(unsigned\s+long\s+long|long\s+long|unsigned\b|\w+)(.*)", re.S)
_DECLARATOR = re.compile(r"\s*((?:\*\s*)*)(\w+)\s*(?:\[([^\]]*)\])?\s*")
_ITEM = re.compile(r"""
    ^[ \t]*\#[ \t]*define[ \t]+(?P<define>\w+)[ \t]+(?P<value>\S.*?)[ \t]*$
  | ^[ \t]*\#[ \t]*(?:include\b.*|ifndef\b.*|endif\b.*|define[ \t]+\w+[ \t]*)$
  | \benum\s*\{(?P<enum>[^{}]*)\}\s*;
  | \btypedef\s+struct\s+(?P<tag>\w+)\s*\{(?P<fields>[^{}]*)\}\s*(?P<struct>\w+)\s*;
  | (?P<result>[\w\s*]+?)\b(?P<function>\w+)\s*\((?P<params>[^(){};]*)\)\s*;
""", re.M | re.X)


def _const_expr(text, consts, where):
    expr = re.sub(r"[A-Za-z_]\w*", lambda m: str(consts[m.group()]) if m.group() in consts else m.group(), text)
    if not re.fullmatch(r"[\d\s+\-*()]+", expr):
        raise RuntimeError("ao_amd: %s: `%s` is not an integer constant expression of known names" % (where, text.strip()))
    try:
        return int(eval(expr, {"__builtins__": {}}))  # (digits, + - * and parentheses only: checked above)
    except SyntaxError:
        raise RuntimeError("ao_amd: %s: cannot evaluate `%s`" % (where, text.strip())) from None


def _declarations(text, structs, consts, where, fields):
    """`const float *q, *key[2]` -> [("q", c_void_p), ("key", c_void_p * 2)]: one type, one or more declarators.  In a
    parameter list (fields False) an array is the pointer it decays to and a struct cannot be passed by value."""
    m = _TYPE.match(re.sub(r"\b(const|volatile)\b", " ", text))
    base = " ".join(m.group(1).split()) if m else None
    out = []
    for decl in m.group(2).split(",") if m else [""]:
        d = _DECLARATOR.fullmatch(decl)
        if d is None:
            raise RuntimeError("ao_amd: %s: cannot read the declaration `%s`" % (where, " ".join(text.split())))
        stars, name, bound = d.group(1).count("*"), d.group(2), d.group(3)
        value = _VALUES.get(base) or (structs.get(base) if fields else None)
        if stars or (bound is not None and not fields):
            if value is None and base not in _POINTEES and base not in structs:
                raise RuntimeError("ao_amd: %s: unknown type `%s` of `%s`" % (where, base, name))
            ctype = ctypes.c_char_p if (base, stars, bound) == ("char", 1, None) else ctypes.c_void_p
        elif value is None:
            raise RuntimeError("ao_amd: %s: no ctypes type for `%s` of `%s`" % (where, base, name))
        else:
            ctype = value
        if bound is not None and fields:
            ctype = ctype * _const_expr(bound, consts, "%s, bound of `%s`" % (where, name))
        out.append((name, ctype))
    return out


def parse(text):
    """(consts, structs, signatures) of a header in the subset described above."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#[ \t]*ifdef[ \t]+__cplusplus\b.*?^[ \t]*#[ \t]*endif\b.*?$", " ", text, flags=re.S | re.M)
    consts, structs, signatures = {}, {}, {}
    at = 0
    for m in _ITEM.finditer(text):
        if text[at:m.start()].strip():
            break
        at = m.end()
        if m.group("define"):
            consts[m.group("define")] = _const_expr(m.group("value"), consts, "#define " + m.group("define"))
        elif m.group("enum") is not None:
            value = -1
            for item in filter(None, (i.strip() for i in m.group("enum").split(","))):
                name, _, init = (s.strip() for s in item.partition("="))
                value = _const_expr(init, consts, "enumerator " + name) if init else value + 1
                consts[name] = value
        elif m.group("struct"):
            name = m.group("struct")
            if name != m.group("tag"):
                raise RuntimeError("ao_amd: typedef struct %s is named %s" % (m.group("tag"), name))
            fields = [f for line in m.group("fields").split(";") if line.strip()
                      for f in _declarations(line, structs, consts, "struct " + name, True)]
            structs[name] = type(name, (ctypes.Structure,), {"_fields_": fields})
        elif m.group("function"):
            name, params = m.group("function"), m.group("params").strip()
            where = "prototype of " + name
            (_, restype), = _declarations(m.group("result") + " result", structs, consts, where, False)
            signatures[name] = (restype, [] if params in ("", "void") else [
                ctype for p in params.split(",") for _, ctype in _declarations(p, structs, consts, where, False)])
    rest = text[at:].strip()
    if rest:
        raise RuntimeError("ao_amd: cannot read this declaration of the C header: `%s`" % " ".join(rest.split())[:160])
    return consts, structs, signatures


if not os.path.exists(HEADER):
    raise RuntimeError("ao_amd: %s not found: the ctypes bindings are derived from it" % HEADER)
with open(HEADER) as _f:
    consts, structs, signatures = parse(_f.read())

# the second public header (the input pipeline's augmentation launchers), read the same way into tables of its own
DATA_HEADER = os.path.join(os.path.dirname(HEADER), "ptv2_data_hip.h")
if not os.path.exists(DATA_HEADER):
    raise RuntimeError("ao_amd: %s not found: the ctypes bindings are derived from it" % DATA_HEADER)
with open(DATA_HEADER) as _f:
    data_consts, data_structs, data_signatures = parse(_f.read())

# the third public header (REAL's epoch-end label refinement), likewise
REFINE_HEADER = os.path.join(os.path.dirname(HEADER), "ptv2_refine_hip.h")
if not os.path.exists(REFINE_HEADER):
    raise RuntimeError("ao_amd: %s not found: the ctypes bindings are derived from it" % REFINE_HEADER)
with open(REFINE_HEADER) as _f:
    refine_consts, refine_structs, refine_signatures = parse(_f.read())

# the fourth public header (the PP2S label pipeline: bridges, weak labels, mask votes), likewise
PP2S_HEADER = os.path.join(os.path.dirname(HEADER), "ptv2_pp2s_hip.h")
if not os.path.exists(PP2S_HEADER):
    raise RuntimeError("ao_amd: %s not found: the ctypes bindings are derived from it" % PP2S_HEADER)
with open(PP2S_HEADER) as _f:
    pp2s_consts, pp2s_structs, pp2s_signatures = parse(_f.read())

# the fifth public header (Point Transformer V1's vector-attention layer), likewise
PTV1_HEADER = os.path.join(os.path.dirname(HEADER), "ptv2_ptv1_hip.h")
if not os.path.exists(PTV1_HEADER):
    raise RuntimeError("ao_amd: %s not found: the ctypes bindings are derived from it" % PTV1_HEADER)
with open(PTV1_HEADER) as _f:
    ptv1_consts, ptv1_structs, ptv1_signatures = parse(_f.read())

# the sixth public header (SpUNet-v1m1's sparse convolutions and their tables), likewise
SPCONV_HEADER = os.path.join(os.path.dirname(HEADER), "ptv2_spconv_hip.h")
if not os.path.exists(SPCONV_HEADER):
    raise RuntimeError("ao_amd: %s not found: the ctypes bindings are derived from it" % SPCONV_HEADER)
with open(SPCONV_HEADER) as _f:
    spconv_consts, spconv_structs, spconv_signatures = parse(_f.read())

# the seventh public header (PointGroup's clustering stage: ball query, clusters, proposals, offset losses), likewise
PG_HEADER = os.path.join(os.path.dirname(HEADER), "ptv2_pg_hip.h")
if not os.path.exists(PG_HEADER):
    raise RuntimeError("ao_amd: %s not found: the ctypes bindings are derived from it" % PG_HEADER)
with open(PG_HEADER) as _f:
    pg_consts, pg_structs, pg_signatures = parse(_f.read())

# the eighth public header (Masked Scene Contrast: InfoNCE over matched pairs, pair matching, patch ids), likewise
MSC_HEADER = os.path.join(os.path.dirname(HEADER), "ptv2_msc_hip.h")
if not os.path.exists(MSC_HEADER):
    raise RuntimeError("ao_amd: %s not found: the ctypes bindings are derived from it" % MSC_HEADER)
with open(MSC_HEADER) as _f:
    msc_consts, msc_structs, msc_signatures = parse(_f.read())

# the ninth public header (Stratified Transformer: window cells, pair lists, the pointops2 attention operators, fused window
# attention), likewise
ST_HEADER = os.path.join(os.path.dirname(HEADER), "ptv2_st_hip.h")
if not os.path.exists(ST_HEADER):
    raise RuntimeError("ao_amd: %s not found: the ctypes bindings are derived from it" % ST_HEADER)
with open(ST_HEADER) as _f:
    st_consts, st_structs, st_signatures = parse(_f.read())

# the tenth public header (the instance-segmentation evaluator's association pass), likewise
INSEVAL_HEADER = os.path.join(os.path.dirname(HEADER), "ptv2_inseval_hip.h")
if not os.path.exists(INSEVAL_HEADER):
    raise RuntimeError("ao_amd: %s not found: the ctypes bindings are derived from it" % INSEVAL_HEADER)
with open(INSEVAL_HEADER) as _f:
    inseval_consts, inseval_structs, inseval_signatures = parse(_f.read())

# the eleventh public header (Masked Scene Contrast v1m2: the partitioned InfoNCE loss of CSC), likewise
CSC_HEADER = os.path.join(os.path.dirname(HEADER), "ptv2_csc_hip.h")
if not os.path.exists(CSC_HEADER):
    raise RuntimeError("ao_amd: %s not found: the ctypes bindings are derived from it" % CSC_HEADER)
with open(CSC_HEADER) as _f:
    csc_consts, csc_structs, csc_signatures = parse(_f.read())

# the twelfth public header (PT-v2m1: the logits stage with GroupedLinear and the position multiplier), likewise
V2M1_HEADER = os.path.join(os.path.dirname(HEADER), "ptv2_v2m1_hip.h")
if not os.path.exists(V2M1_HEADER):
    raise RuntimeError("ao_amd: %s not found: the ctypes bindings are derived from it" % V2M1_HEADER)
with open(V2M1_HEADER) as _f:
    v2m1_consts, v2m1_structs, v2m1_signatures = parse(_f.read())
