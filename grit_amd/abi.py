"""The C ABI of libgrit_hip.so as data, read from include/grit_hip.h: the one place where it is written down.

No torch, no library.  `read()` returns an Abi of
  functions   name -> (restype, [argtypes])
  structs     name -> [(field, ctype)]                the `typedef struct [tag] { ... } name;` blocks, fields in order
  constants   name -> int                             the `#define NAME <integer>` lines; macros with arguments are not constants
  version     constants["GRIT_ABI_VERSION"]
The reader knows the subset of C that the header uses and nothing more; whatever it cannot fully parse raises AbiError with the
declaration in the message -- an unknown type, a nested struct, a function pointer, a missing `;`.  That refusal is what keeps the
header inside the subset.
"""
import collections
import ctypes
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "grit_hip.h")

SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double,
           "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "unsigned long long": ctypes.c_ulonglong}
POINTEES = set(SCALARS) | {"void", "char", "unsigned char", "unsigned int", "int32_t", "uint32_t", "uint8_t"}  # + the structs

Abi = collections.namedtuple("Abi", "functions structs constants version")


class AbiError(ValueError):
    pass


def _ctype(tokens, decl, structs, returned=False):
    """ctypes type of a declarator-free C type given as tokens (`const`, type words, `*`)."""
    words = [t for t in tokens if t not in ("const", "*")]
    base, stars = " ".join(words), tokens.count("*")
    if "*" in tokens and [t for t in tokens[tokens.index("*"):] if t not in ("const", "*")]:
        raise AbiError("cannot parse the type of `%s`" % decl)
    if stars:
        if base not in POINTEES and base not in structs:
            raise AbiError("unknown type `%s` in `%s`" % (base, decl))
        return ctypes.c_char_p if (returned and base == "char" and stars == 1) else ctypes.c_void_p
    if base not in SCALARS:
        raise AbiError("unknown type `%s` in `%s`" % (base, decl))
    return SCALARS[base]


def _declarator(text, decl, structs):
    """(name, ctype) of `type name`, `type* name`, `type name[]` (a pointer) or `type name[N]` (an array)."""
    if "(" in text or "{" in text or re.search(r"\bstruct\b", text):
        raise AbiError("function pointers and nested structs are not part of the ABI: `%s`" % decl)
    m = re.fullmatch(r"\s*((?:\w+|\*|\s)+?)\s*\b(\w+)\s*(?:\[\s*(\d*)\s*\])?\s*", text)
    if not m or not m.group(1).strip():
        raise AbiError("cannot parse `%s` in `%s`" % (text.strip(), decl))
    tokens, name, count = re.findall(r"\w+|\*", m.group(1)), m.group(2), m.group(3)
    if count == "":
        tokens = tokens + ["*"]
    ctype = _ctype(tokens, decl, structs)
    return name, (ctype * int(count) if count else ctype)


def _prototype(decl, structs):
    m = re.fullmatch(r"((?:\w+|\*|\s)+?)\s*\b(\w+)\s*\((.*)\)", decl, flags=re.S)
    if not m:
        raise AbiError("cannot parse the declaration `%s`" % decl)
    restype = None if m.group(1).strip() == "void" else _ctype(re.findall(r"\w+|\*", m.group(1)), decl, structs, returned=True)
    params = m.group(3).strip()
    argtypes = [] if params in ("void", "") else [_declarator(p, decl, structs)[1] for p in params.split(",")]
    if any(isinstance(a, type) and issubclass(a, ctypes.Array) for a in argtypes):
        raise AbiError("sized array parameter in `%s`" % decl)
    return m.group(2), (restype, argtypes)


def _struct(decl, structs):
    m = re.fullmatch(r"typedef\s+struct\s*(\w*)\s*\{(.*)\}\s*(\w+)", decl, flags=re.S)
    if not m or (m.group(1) and m.group(1) != m.group(3)):
        raise AbiError("cannot parse the struct `%s`" % decl)
    fields = []
    for member in m.group(2).split(";")[:-1]:
        first, *more = member.split(",")
        fields.append(_declarator(first, member.strip(), structs))
        for extra in more:  # `int a, b, c;`: plain names (or arrays) of a pointer-free type
            if "*" in member or not re.fullmatch(r"\s*\w+\s*(\[\s*\d+\s*\])?\s*", extra):
                raise AbiError("cannot parse `%s` in struct %s" % (member.strip(), m.group(3)))
            fields.append(_declarator(first.rsplit(None, 1)[0] + " " + extra, member.strip(), structs))
    if m.group(2).split(";")[-1].strip() or not fields:
        raise AbiError("cannot parse the struct `%s`" % decl)
    return m.group(3), fields


def parse(text):
    """Abi of a header given as text."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text).replace("\\\n", " ")
    constants, code, skipping = {}, [], []
    for line in text.split("\n"):
        if not line.lstrip().startswith("#"):
            code.append("" if any(skipping) else line)
            continue
        directive = line.strip()[1:].split()
        if directive[0] in ("ifdef", "ifndef") and len(directive) == 2:
            skipping.append(directive == ["ifdef", "__cplusplus"])  # the extern "C" braces: not C
        elif directive == ["endif"] and skipping:
            skipping.pop()
        elif directive[0] == "define" and re.fullmatch(r"\w+", directive[1]):
            if len(directive) == 3 and re.fullmatch(r"-?(0[xX][0-9a-fA-F]+|\d+)", directive[2]):
                constants[directive[1]] = int(directive[2], 0)
            elif len(directive) != 2:  # two words: an include guard
                raise AbiError("`%s` is not an integer constant" % line.strip())
        elif not (directive[0] == "include" or (directive[0] == "define" and re.match(r"\w+\(", directive[1]))):
            raise AbiError("cannot parse the directive `%s`" % line.strip())
    if skipping:
        raise AbiError("unterminated #if block")
    functions, structs = {}, {}
    code, decls, depth, start = "\n".join(code), [], 0, 0
    for i, ch in enumerate(code):  # a `;` outside braces ends a declaration
        depth += (ch == "{") - (ch == "}")
        if ch == ";" and depth == 0:
            decls.append(code[start:i])
            start = i + 1
    if code[start:].strip():
        raise AbiError("unterminated declaration `%s`" % " ".join(code[start:].split()))
    for decl in (" ".join(d.split()) for d in decls):
        if decl.startswith("typedef"):
            name, fields = _struct(decl, structs)
            structs[name] = fields
        elif decl:
            name, signature = _prototype(decl, structs)
            functions[name] = signature
    return Abi(functions, structs, constants, constants.get("GRIT_ABI_VERSION"))


def read(path=HEADER):
    with open(path) as f:
        return parse(f.read())
