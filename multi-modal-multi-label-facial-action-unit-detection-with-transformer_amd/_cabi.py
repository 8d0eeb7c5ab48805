"""Reader of include/avformer_hip.h: the one written declaration of the C ABI, as ctypes types.

The compiler checks every definition in csrc/ against the header; `_lib`, `ops` and `metrics` take their signatures,
structures and constants from here, so there is no second copy to keep in step.  Pure Python, no torch, no library.

The reader knows the few forms the header is written in and REFUSES everything else (HeaderError naming the
declaration): a declaration it skipped would be an entry point called with guessed types.
"""
from __future__ import annotations

import ctypes as C
import functools
import re

from ._build import ABI_HEADER

SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "size_t": C.c_size_t,
           "float": C.c_float, "double": C.c_double, "uint8_t": C.c_uint8}
POINTEES = set(SCALARS) | {"void", "char"}  # what a pointer may point to, besides the header's own structs

_INT = r"-?(?:0[xX][0-9a-fA-F]+|\d+)"
_DEFINE = re.compile(rf"#\s*define\s+(AVF_\w+)\s+({_INT})\s*$")
_PREPROCESSOR_NOISE = re.compile(r"#\s*(?:include\s*<[\w./]+>|ifndef\s+\w+|ifdef\s+__cplusplus|endif|define\s+(?!AVF_)\w+)\s*$")
_STRUCT = re.compile(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;")
_ENUM = re.compile(r"enum\s*\{([^{}]*)\}\s*;")
_PROTO = re.compile(r"([\w\s*]+?)\b(\w+)\s*\(([\w\s*,]*)\)\s*;")
_ENUMERATOR = re.compile(rf"\s*(AVF_\w+)\s*=\s*({_INT})\s*$")
_TOKEN = re.compile(r"\w+|\*|\[|\]")
_SPACE = re.compile(r"\s*")
_IDENTIFIER = re.compile(r"[A-Za-z_]\w*")


class HeaderError(ValueError):
    pass


def _type(tokens, structs, decl):
    """(`const`, words and stars of one type) -> ctypes type; a pointer to one of the header's structs -> its name"""
    words = [t for t in tokens if t not in ("*", "const")]
    stars = tokens.count("*")
    base = " ".join(words)
    if len(words) != 1 or (base not in POINTEES and base not in structs):
        raise HeaderError(f"unknown type {base!r} in: {decl}")
    if stars == 0:
        if base not in SCALARS:
            raise HeaderError(f"{base!r} by value in: {decl}")
        return SCALARS[base]
    if stars == 1 and base in structs:
        return base
    if stars == 1 and base == "char" and tokens[0] == "const":
        return C.c_char_p
    return C.c_void_p


def _name(token, decl):
    if not _IDENTIFIER.fullmatch(token) or token in POINTEES or token == "const":
        raise HeaderError(f"a declarator without a name in: {decl}")
    return token


def _fields(body, defines, structs, decl):
    fields = []
    for member in filter(None, (m.strip() for m in body.split(";"))):
        if not re.fullmatch(r"[\w\s*,\[\]]+", member):  # a bit-field's ':', a function pointer's '(' ...
            raise HeaderError(f"unsupported member {member!r} in: {decl}")
        base = None
        for part in member.split(","):
            tokens = _TOKEN.findall(part)
            count = None
            if tokens[-1:] == ["]"]:
                if len(tokens) < 4 or tokens[-3] != "[":
                    raise HeaderError(f"unsupported array {member!r} in: {decl}")
                length = tokens[-2]
                count = defines[length] if length in defines else int(length) if re.fullmatch(r"\d+", length) else None
                if count is None or count <= 0:
                    raise HeaderError(f"array length {length!r} is neither a literal nor an AVF_* define in: {decl}")
                tokens = tokens[:-3]
            if not tokens:
                raise HeaderError(f"empty declarator {member!r} in: {decl}")
            name, tokens = _name(tokens[-1], member), tokens[:-1]
            if base is None:  # the first declarator carries the type words; every declarator its own stars
                base = [t for t in tokens if t != "*"]
            elif any(t != "*" for t in tokens):
                raise HeaderError(f"unsupported declarator {part.strip()!r} in: {decl}")
            ctype = _type(base + ["*"] * tokens.count("*"), structs, member)
            if isinstance(ctype, str) or ctype is C.c_char_p:
                ctype = C.c_void_p  # pointer fields are plain addresses
            fields.append((name, ctype * count if count else ctype))
    if not fields:
        raise HeaderError(f"empty struct: {decl}")
    return fields


def parse(path):
    """-> (defines, structs, functions) of the header at `path`:
    defines    {name: int} of every `#define AVF_<NAME> <integer>` and every enumerator of an anonymous enum;
    structs    {name: [(field, ctype), ...]} in declaration order (pointer fields are c_void_p);
    functions  {name: (restype, [argtypes])}.  Scalars are their ctypes types, `const char*` is c_char_p, a pointer to one of
               the header's structs is that struct's NAME (bind() turns it into POINTER(Structure)), and every other pointer
               is c_void_p: callers pass data_ptr() integers, byref() and ctypes arrays through them."""
    with open(path) as f:
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", f.read(), flags=re.S)
    defines, structs, functions = {}, {}, {}
    code, in_cplusplus = [], False
    for line in text.split("\n"):
        s = line.strip()
        if s.startswith("#"):
            m = _DEFINE.match(s)
            if m:
                defines[m.group(1)] = int(m.group(2), 0)
            elif not _PREPROCESSOR_NOISE.match(s):
                raise HeaderError(f"unsupported preprocessor line: {s}")
            in_cplusplus = s.replace(" ", "") == "#ifdef__cplusplus"
        elif in_cplusplus:
            if s not in ('extern "C" {', "}", ""):
                raise HeaderError(f"unsupported line under #ifdef __cplusplus: {s}")
        else:
            code.append(line)
    text = "\n".join(code)
    pos = 0
    while True:
        pos = _SPACE.match(text, pos).end()
        if pos == len(text):
            break
        decl = " ".join(text[pos:text.find(";", pos) + 1 or len(text)].split())
        if m := _STRUCT.match(text, pos):
            if m.group(1) != m.group(3) or m.group(1) in structs:
                raise HeaderError(f"struct tag and typedef name differ, or a second definition: {decl}")
            structs[m.group(1)] = _fields(m.group(2), defines, structs, f"struct {m.group(1)}")
        elif m := _ENUM.match(text, pos):
            for item in m.group(1).split(","):
                e = _ENUMERATOR.match(item)
                if not e:
                    raise HeaderError(f"enumerator {item.strip()!r} is not AVF_<NAME> = <integer> in: {decl}")
                defines[e.group(1)] = int(e.group(2), 0)
        elif m := _PROTO.match(text, pos):
            name = m.group(2)
            if not name.startswith("avf_") or name in functions:
                raise HeaderError(f"not an avf_ entry point, or declared twice: {decl}")
            ret = _TOKEN.findall(m.group(1))
            args = []
            if m.group(3).strip() != "void":
                for param in m.group(3).split(","):
                    tokens = _TOKEN.findall(param)
                    if len(tokens) < 2:
                        raise HeaderError(f"a parameter without a name in: {decl}")
                    _name(tokens[-1], decl)
                    args.append(_type(tokens[:-1], structs, decl))
            functions[name] = (_type(ret, structs, decl), args)
        else:
            raise HeaderError(f"unsupported declaration: {decl}")
        pos = m.end()
    return defines, structs, functions


def bind(functions, structures):
    """`functions` of parse() with every struct name replaced by POINTER(structures[name])"""
    return {name: (res, [C.POINTER(structures[a]) if isinstance(a, str) else a for a in args])
            for name, (res, args) in functions.items()}


@functools.lru_cache(maxsize=None)
def header():
    """parse(ABI_HEADER), read once per process at the first use"""
    return parse(ABI_HEADER)
