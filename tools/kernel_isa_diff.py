#!/usr/bin/env python3
"""Compare the gfx950 device code of two source trees, kernel by kernel: the acceptance check of a refactor of the GEMM units.

    tools/kernel_isa_diff.py <old tree> <new tree> [unit ...]        # units: gemm_bf16_v2 gemm_fp8 ...; default: every csrc/*.hip
    tools/kernel_isa_diff.py <old tree> <new tree> --units gemm_skinny_fp8+gemm_skinny_fp4=gemm_skinny_mx      # units that were merged

Each unit of both trees is compiled with the FLAGS of its own tree's csrc/Makefile plus `--cuda-device-only -S`; comments and the
per-build `__hip_cuid_*` symbol are dropped, the compiler's running function numbers in local labels are blanked, and the text
of every device function (code, kernel descriptor, metadata record) is compared.  One line per function: `identical`,
`DIFFERENT`, `removed` or `added`; exit status 1 if anything is DIFFERENT.  --map rewrites mangled names of the OLD tree
before matching (a template parameter that went away); the gg8_kernel MODE parameter is built in.  --units OLD+OLD=NEW compares
the new unit with the union of the named old ones, whose `(module data)` is reported as `merged` and not counted.  --keep DIR keeps the
assembly there and reuses a listing that is newer than its tree's sources.  It compares two builds with each other and nothing
else."""
import argparse, concurrent.futures, difflib, os, re, subprocess, sys, tempfile

MAX_JOBS = 16
# old mangled name -> new: gg8_kernel<ROWK, COLK, MODE = 0, SCHED, ACC> lost MODE
BUILTIN_MAPS = [(r"(10gg8_kernelILi\d+ELi\d+E)Li0E(Li\d+ELb[01]EE)", r"\1\2")]
HEADER = re.compile(r"\t\.(text|section\t\.text|globl|weak|protected|hidden|p2align)\b")


def csrc(tree):
    return os.path.join(tree, "competesmoe_amd", "csrc")


def flags(tree):
    mk = open(os.path.join(csrc(tree), "Makefile")).read()
    var = dict(re.findall(r"^(\w+)\s*[:?]?=\s*(.*)$", mk, re.M))
    return re.sub(r"\$\((\w+)\)", lambda m: var[m.group(1)], var["FLAGS"]).split(), var["HIPCC"]


def compile_unit(tree, unit, out):
    src = csrc(tree)
    deps = [os.path.join(src, f) for f in os.listdir(src)] + [os.path.join(tree, "include", "csmoe.h")]
    if os.path.exists(out) and os.path.getmtime(out) > max(os.path.getmtime(d) for d in deps):
        return
    fl, hipcc = flags(tree)
    r = subprocess.run([os.environ.get("HIPCC", hipcc)] + fl + ["--cuda-device-only", "-S", unit + ".hip", "-o", out + ".tmp"],
                       cwd=src, capture_output=True, text=True)
    if r.returncode:
        sys.exit(f"{tree}: {unit}.hip does not compile\n{r.stderr}")
    os.replace(out + ".tmp", out)


def functions(path, maps):
    """{function name: normalised text}; everything outside a function is under '(module data)'."""
    out, cur, pending, in_meta = {"(module data)": []}, "(module data)", [], False
    for ln in open(path):
        ln = ln.rstrip("\n")
        if '"' not in ln:
            ln = ln.split(";", 1)[0].rstrip()
        if not ln.strip() or "__hip_cuid_" in ln:
            continue
        for pat, rep in maps:
            ln = re.sub(pat, rep, ln)
        ln = re.sub(r"\.L(BB|func_begin|func_end|tmp)\d+", r".L\1", ln)
        m = re.match(r"\t\.type\t(\S+),@function", ln)
        if m:
            cur = m.group(1)
            out[cur] = pending
            pending = []
        elif re.match(r"\t\.section\t\.AMDGPU\.gpr_maximums|\t\.amdgpu_metadata", ln):
            cur, in_meta = "(module data)", in_meta or "metadata" in ln
        elif in_meta and ln.startswith("  - ."):
            cur = pending = []                      # a kernel's metadata record: filed under its .name once that is read
        elif in_meta and not ln.startswith("   "):
            cur = "(module data)"
        if HEADER.match(ln) and not isinstance(cur, list):
            pending.append(ln)                      # the lines in front of a function's .type belong to that function
            continue
        if isinstance(cur, list):
            cur.append(ln)
            m = re.match(r"    \.name:\s+(\S+)", ln)
            if m:
                out.setdefault(m.group(1), []).extend(cur)
                cur = m.group(1)
                pending = []
        else:
            out[cur].extend(pending + [ln])
            pending = []
    out["(module data)"] += pending
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
        return dict(zip(names, [d.replace("(anonymous namespace)::", "") for d in r.stdout.split("\n")]))
    except OSError:
        return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old"), ap.add_argument("new"), ap.add_argument("units", nargs="*")
    ap.add_argument("-j", "--jobs", type=int, default=min(MAX_JOBS, os.cpu_count() or 1))
    ap.add_argument("--map", action="append", default=[], metavar="REGEX=REPL", help="rewrite names of the old tree")
    ap.add_argument("--units", dest="merged", action="append", default=[], metavar="OLD+OLD=NEW", help="old units merged into a new one")
    ap.add_argument("--keep", metavar="DIR", help="keep (and reuse) the assembly listings here")
    ap.add_argument("--show", type=int, default=0, metavar="N", help="print the first N diff lines of a DIFFERENT function")
    a = ap.parse_args()
    units = [u[:-4] if u.endswith(".hip") else u for u in a.units] or \
        sorted(f[:-4] for f in os.listdir(csrc(a.new)) if f.endswith(".hip"))
    work = a.keep or tempfile.mkdtemp(prefix="isa_diff_")
    maps = BUILTIN_MAPS + [tuple(m.split("=", 1)) for m in a.map]
    merged = {new: old.split("+") for old, new in (m.split("=", 1) for m in a.merged)}
    jobs = [(a.new, u, os.path.join(work, "new", u + ".s")) for u in units] + \
        [(a.old, o, os.path.join(work, "old", o + ".s")) for u in units for o in merged.get(u, [u])]
    for side in ("old", "new"):
        os.makedirs(os.path.join(work, side), exist_ok=True)
    with concurrent.futures.ThreadPoolExecutor(max(1, min(a.jobs, MAX_JOBS))) as ex:
        list(ex.map(lambda j: compile_unit(*j), jobs))
    bad = 0
    for u in units:
        old = {}
        for o in merged.get(u, [u]):
            for n, text in functions(os.path.join(work, "old", o + ".s"), maps).items():
                old.setdefault(n, []).extend(text)
        new = functions(os.path.join(work, "new", u + ".s"), [])
        names = list(dict.fromkeys(list(old) + list(new)))
        pretty = demangle(names)
        for n in names:
            if n not in new or n not in old:
                verdict = "removed" if n in old else "added"
            else:
                verdict = "identical" if old[n] == new[n] else "DIFFERENT"
            if verdict == "DIFFERENT" and u in merged and n == "(module data)":
                verdict = "merged"                  # the old units' records one after the other: shown, not counted
            bad += verdict == "DIFFERENT"
            lines = f"{len(new[n]) if n in new else len(old[n])} lines"
            print(f"{u:18s} {verdict:10s} {pretty[n]}  ({lines})")
            if verdict == "DIFFERENT" and a.show:
                print("\n".join(list(difflib.unified_diff(old[n], new[n], "old", "new", lineterm="", n=1))[:a.show]))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
