"""Compares the gfx950 device code of two trees, symbol by symbol: the proof that a host-side
change left every kernel as it was.

    python tools/device_code_diff.py emit OUTDIR     compiles every build_native.SOURCES entry of this
                                                     tree with build_native.FLAGS to OUTDIR/<name>.s
    python tools/device_code_diff.py compare A B     compares two such directories

Per file the listing is split into each @function symbol's body (label to .Lfunc_end), each
.amdhsa_kernel block, each kernel's .amdgpu_metadata entry and each @object symbol's size.  What
depends only on emission order or on the compile is normalised: the function index in .LBB<n>_<m>,
.LJTI<n>_<m>, .Lfunc_begin<n>, .Lfunc_end<n> and the BB<n>_<m> of loop comments, the numbers of
.Ltmp labels (renumbered by first use in the symbol), the __hip_cuid_* symbol, runs of blanks (the
padding of a label's comment follows the index's width); .ident and .file lie
outside every symbol.  The symbols only in A, only in B or different are printed; exit status 1 if
there are any.  Text is compared: no instruction is named."""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
_INDEXED = re.compile(r"(\.LBB|\bBB|\.LJTI|\.Lfunc_begin|\.Lfunc_end)\d+")
_TMP = re.compile(r"\.Ltmp\d+")
_CUID = re.compile(r"__hip_cuid_[0-9a-f]+")
_BLANKS = re.compile(r"[ \t]+")
_TYPE = re.compile(r"\.type\s+([^,\s]+),@(function|object)")
_LABEL = re.compile(r"([A-Za-z_$][\w$.]*):")
_SIZE = re.compile(r"\.size\s+([^,\s]+),\s*(\d+)$")
_MD_NAME = re.compile(r"    \.name:\s+(\S+)")


def normalise(lines):
    tmp = {}
    out = []
    for ln in lines:
        # (blanks: the compiler pads a label's comment to a column, so the padding follows the index's digits)
        ln = _BLANKS.sub(" ", _CUID.sub("__hip_cuid_", _INDEXED.sub(r"\1", ln.strip())))
        out.append(_TMP.sub(lambda m: tmp.setdefault(m.group(0), ".Ltmp%d" % len(tmp)), ln))
    return out


def split(text):
    """{"fn:" / "kd:" / "md:" / "obj:" + symbol -> normalised lines} of one listing: function bodies,
    kernel descriptors, metadata entries, object sizes"""
    syms, types = {}, {}
    fn = kd = md = None    # the open function body, kernel descriptor, metadata entry: (name, lines)
    in_md = False

    def close_md():
        if md:
            name = next((m.group(1) for m in map(_MD_NAME.match, md) if m), "?")
            syms["md:" + name] = normalise(md)

    for ln in text.splitlines():
        t = ln.strip()
        if in_md:                                  # the kernels' list of .amdgpu_metadata (YAML)
            if ln.startswith("  - "):              # the next kernel's entry
                close_md()
                md = [ln]
            elif ln.startswith(" "):
                md.append(ln)
            else:                                  # amdhsa.target: the list is over
                close_md()
                md, in_md = None, False
            continue
        if ln.startswith("amdhsa.kernels"):
            in_md = True
        elif kd is not None:
            if t == ".end_amdhsa_kernel":
                syms["kd:" + kd[0]] = normalise(kd[1])
                kd = None
            else:
                kd[1].append(t)
        elif t.startswith(".amdhsa_kernel "):
            kd = (t.split()[1], [])
        elif _TYPE.match(t):
            m = _TYPE.match(t)
            types[m.group(1)] = m.group(2)
        elif _SIZE.match(t) and types.get(_SIZE.match(t).group(1)) == "object":
            m = _SIZE.match(t)
            syms["obj:" + _CUID.sub("__hip_cuid_", m.group(1))] = [m.group(2)]
        elif fn is None and _LABEL.match(ln) and types.get(_LABEL.match(ln).group(1)) == "function":
            fn = (_LABEL.match(ln).group(1), [])
        elif fn is not None:
            if re.match(r"\.Lfunc_end\d+:", t):
                syms["fn:" + fn[0]] = normalise(fn[1])
                fn = None
            elif t:
                fn[1].append(t)
    return syms


def compare_text(a, b):
    """(only in a, only in b, different) symbol lists of two listings"""
    sa, sb = split(a), split(b)
    return (sorted(set(sa) - set(sb)), sorted(set(sb) - set(sa)),
            sorted(k for k in set(sa) & set(sb) if sa[k] != sb[k]))


def emit(outdir):
    sys.path.insert(0, os.path.dirname(HERE))
    from pytorch_hmm_amd import build_native as bn
    os.makedirs(outdir, exist_ok=True)

    def one(s):
        cmd = [bn._hipcc(), *bn.FLAGS, "--cuda-device-only", "-S", os.path.join(bn.CSRC, s), "-o",
               os.path.join(outdir, s.replace(".hip", ".s"))]
        subprocess.run(cmd, check=True)

    with ThreadPoolExecutor(max_workers=8) as ex:
        list(ex.map(one, bn.SOURCES))
    return 0


def compare(da, db):
    bad = 0
    names = sorted({f for d in (da, db) for f in os.listdir(d) if f.endswith(".s")})
    for f in names:
        pa, pb = os.path.join(da, f), os.path.join(db, f)
        if not (os.path.exists(pa) and os.path.exists(pb)):
            print(f"{f}: only in {da if os.path.exists(pa) else db}")
            bad += 1
            continue
        with open(pa) as fa, open(pb) as fb:
            ta, tb = fa.read(), fb.read()
        only_a, only_b, diff = compare_text(ta, tb)
        for tag, ks in (("only in A", only_a), ("only in B", only_b), ("differs", diff)):
            for k in ks:
                print(f"{f}: {tag}: {k}")
        n = {kind: sum(1 for k in split(tb) if k.startswith(kind + ":")) for kind in ("fn", "kd", "obj")}
        nd = len(only_a) + len(only_b) + len(diff)
        print(f"{f}: {n['kd']} kernels, {n['fn']} functions, {n['obj']} objects compared, {nd} differences")
        bad += nd
    print(f"{len(names)} translation units, " + ("no difference" if bad == 0 else f"{bad} differences"))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "emit":
        sys.exit(emit(sys.argv[2]))
    if len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    sys.exit(__doc__)
