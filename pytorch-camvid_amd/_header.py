"""Reader of include/cvk.h: the header is the one place the C boundary is written down, and the ctypes side is derived from it.

    h = read(path)            # or parse(text)
    h.prototypes              # name -> (restype, [argtypes])
    h.structs                 # name -> ctypes.Structure subclass with the header's field names
    h.defines                 # NAME -> int, for `#define NAME <integer literal>`

Pure Python: no torch, no library load.  The reader knows the closed type map below and the declaration forms the header uses
(prototypes, `typedef struct NAME { ... } NAME;`, integer defines).  Anything else raises CvkError naming the declaration: a
binding that guessed would pass garbage to a kernel launch."""
import collections
import ctypes
import re


class CvkError(RuntimeError):
    pass


SCALARS = {
    "int": ctypes.c_int, "long": ctypes.c_long, "unsigned": ctypes.c_uint, "float": ctypes.c_float, "double": ctypes.c_double,
    "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint8_t": ctypes.c_uint8, "uint64_t": ctypes.c_uint64,
    "size_t": ctypes.c_size_t, "unsigned long long": ctypes.c_ulonglong,
}
POINTEES = set(SCALARS) | {"void", "char", "unsigned char", "uint32_t"}     # what a pointer may point to, besides a struct of the header
TYPE_WORDS = {w for t in POINTEES for w in t.split()} | {"const", "struct"}

Header = collections.namedtuple("Header", "prototypes structs defines")

_INT = r"-?\s*(?:0[xX][0-9a-fA-F]+|[1-9][0-9]*|0)"
_DEFINE = re.compile(rf"\s*#\s*define\s+(\w+)\s+(?:({_INT})|\(\s*({_INT})\s*\))\s*")
_NAME = r"[A-Za-z_]\w*"


def strip_comments(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def _ctype(spec, structs, decl, ret=False):
    """ctypes type of a C type written as `spec` (no declarator name in it)."""
    words = spec.replace("*", " * ").split()
    const = "const" in words
    words = [w for w in words if w != "const"]
    stars = words.count("*")
    if stars and words[-stars:] != ["*"] * stars:
        raise CvkError(f"cvk.h: cannot take the type '{spec}' apart in: {decl}")
    base = " ".join(words[:len(words) - stars])
    if stars:
        if base not in POINTEES and base not in structs:
            raise CvkError(f"cvk.h: pointer to the unknown type '{base}' in: {decl}")
        if not ret:
            return ctypes.c_void_p
        if stars == 1 and base == "char" and const:
            return ctypes.c_char_p
        if stars == 1 and base == "void":
            return ctypes.c_void_p
        raise CvkError(f"cvk.h: no mapping for the return type '{spec}' in: {decl}")
    if ret and base == "void":
        return None
    if base in SCALARS:
        return SCALARS[base]
    if base in structs:
        return structs[base]
    raise CvkError(f"cvk.h: unknown type '{base}' (a struct passed by value is known only after, not before its definition) in: {decl}")


def _split_name(text, decl):
    """`const float* x` -> (`const float*`, `x`).  The name is required, so that `unsigned long` is never read as a `long` named so."""
    m = re.fullmatch(rf"(.*[\s*])({_NAME})", text.strip(), flags=re.S)
    if not m or m.group(2) in TYPE_WORDS or not m.group(1).strip():
        raise CvkError(f"cvk.h: expected '<type> <name>', found '{text.strip()}' in: {decl}")
    return m.group(1).strip(), m.group(2)


def _refuse_forms(text, decl):
    for mark, what in (("...", "a variadic list"), ("(", "a function pointer"), (":", "a bit-field"), ("{", "a nested struct")):
        if mark in text:
            raise CvkError(f"cvk.h: {what} is not supported: {decl}")


def _prototype(decl, structs):
    m = re.fullmatch(rf"(.*?[\s*])({_NAME})\s*\((.*)\)", decl, flags=re.S)
    if not m:
        raise CvkError(f"cvk.h: neither a prototype nor a typedef struct: {decl}")
    ret, name, params = m.groups()
    _refuse_forms(params, decl)
    if "[" in params:
        raise CvkError(f"cvk.h: an array parameter is not supported: {decl}")
    res = _ctype(ret, structs, decl, ret=True)
    if params.strip() == "void":
        return name, (res, [])
    return name, (res, [_ctype(_split_name(p, decl)[0], structs, decl) for p in params.split(",")])


def _struct(decl, structs):
    m = re.fullmatch(rf"typedef\s+struct\s+({_NAME})?\s*\{{(.*)\}}\s*({_NAME})", decl, flags=re.S)
    if not m:
        raise CvkError(f"cvk.h: neither a prototype nor a typedef struct: {decl}")
    short = " ".join(decl.split())
    fields = []
    for line in m.group(2).split(";"):
        if not line.strip():
            continue
        _refuse_forms(line, short)
        first, *more = line.split(",")
        spec, _ = _split_name(first.split("[")[0], short)
        if more and "*" in spec:
            raise CvkError(f"cvk.h: declare one pointer per line, not '{' '.join(line.split())}' in: {short}")
        ctype = _ctype(spec, structs, short)
        for item in [first.strip()[len(spec):]] + more:
            f = re.fullmatch(rf"\s*({_NAME})\s*(?:\[\s*([0-9]+)\s*\])?\s*", item)
            if not f:
                raise CvkError(f"cvk.h: cannot take the field '{item.strip()}' apart in: {short}")
            fields.append((f.group(1), ctype * int(f.group(2)) if f.group(2) else ctype))
    return m.group(3), type(m.group(3), (ctypes.Structure,), {"_fields_": fields})


def _declarations(body):
    """Split at the `;` outside braces."""
    depth, start = 0, 0
    for i, ch in enumerate(body):
        depth += (ch == "{") - (ch == "}")
        if depth < 0:
            raise CvkError("cvk.h: unbalanced '}'")
        if ch == ";" and depth == 0:
            yield body[start:i].strip()
            start = i + 1
    if body[start:].strip():
        raise CvkError(f"cvk.h: text after the last declaration: {' '.join(body[start:].split())[:120]}")


def parse(text):
    text = strip_comments(text).replace("\\\n", " ")
    defines, lines = {}, []
    for line in text.split("\n"):
        if line.lstrip().startswith("#"):
            m = _DEFINE.fullmatch(line)
            if m:
                defines[m.group(1)] = int((m.group(2) or m.group(3)).replace(" ", ""), 0)
            line = ""
        lines.append(line)
    body, opened = re.subn(r'extern\s+"C"\s*\{', " ", "\n".join(lines), count=1)
    if opened:                                   # its closing brace is the last thing in the header
        body = body.rstrip()
        if not body.endswith("}"):
            raise CvkError('cvk.h: extern "C" { is not closed at the end of the header')
        body = body[:-1]
    prototypes, structs = {}, {}
    for decl in _declarations(body):
        if not decl:
            continue
        if decl.startswith("typedef"):
            name, cls = _struct(decl, structs)
            structs[name] = cls
        else:
            name, sig = _prototype(" ".join(decl.split()), structs)
            if name in prototypes:
                raise CvkError(f"cvk.h: {name} is declared twice")
            prototypes[name] = sig
    called = set(re.findall(rf"\b({_NAME})\s*\(", body))      # cross-check with an independent scan: nothing was skipped
    if called != set(prototypes):
        raise CvkError(f"cvk.h: prototypes the reader missed or invented: {sorted(called ^ set(prototypes))}")
    return Header(prototypes, structs, defines)


def read(path):
    try:
        with open(path, encoding="utf-8") as f:
            text = f.read()
    except OSError as e:
        raise CvkError(f"cannot read the C header at {path} ({e.strerror or e}): include/cvk.h ships with the repository, next "
                       "to the package directory, and the ctypes binding is derived from it") from None
    return parse(text)
