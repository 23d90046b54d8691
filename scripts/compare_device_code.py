#!/usr/bin/env python3
"""Is the device code of two source trees the same code?  No GPU needed.

    python scripts/compare_device_code.py TREE_A TREE_B [--jobs N] [--keep DIR]

For each of the four device translation units of libagimus_hip.so (agimus_hip.hip as capacity group 0 and as group 1 with the
rename flags of backend.build(), agx_cost_pairs.hip, agx_diag.hip) both trees are compiled with `--cuda-device-only -S` and the
flags of the build.  The assembly is cut into functions keyed by their mangled name (moving host code changes the order in which
template instantiations are emitted) and compared as plain text after two artefacts of the compile are normalised: the
`__hip_cuid_<hash>` symbol, which depends on the directory a source is compiled from, and the function index in local labels
(`.LBB<n>_<k>` and the `BB<n>_<k>` of the loop comments, `.Lfunc_end<n>`, `.LJTI<n>_<k>`, and the padding in front of a
label's comment, which follows the width of that index).  The `-Rpass-analysis=kernel-resource-usage` remarks of the same
compiles are compared per kernel too (registers, scratch, LDS, occupancy).  Prints the count of kernels per unit and every name that differs; exit status 1 if anything does."""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import importlib.util
import os
import pathlib
import re
import subprocess
import sys
import tempfile

UNITS = ("group0", "group1", "cost_pairs", "diag")


def unit_command(tree: pathlib.Path, unit: str):
    csrc, inc = tree / "agimus_controller_amd" / "csrc", tree / "include"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    base = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{inc}"]
    if unit.startswith("group"):
        spec = importlib.util.spec_from_file_location("agx_front", csrc / "agx_front.py")
        front = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(front)
        names = [n for _, n, _ in front.prototypes((inc / "agimus_hip.h").read_text())]
        return base + front.rename_flags(names, int(unit[-1])) + [str(csrc / "agimus_hip.hip")]
    if unit == "cost_pairs":
        return base + ["-DAGX_GROUP=0", str(csrc / "agx_cost_pairs.hip")]
    return base + [str(csrc / "agx_diag.hip")]


def compile_unit(tree: str, unit: str, out: str):
    cmd = unit_command(pathlib.Path(tree), unit) + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError(f"{unit} of {tree}: hipcc failed\n{res.stderr[-3000:]}")
    pathlib.Path(out + ".remarks").write_text(res.stderr)
    return out


_NORMALISE = ((re.compile(r"__hip_cuid_[0-9a-f]+"), "__hip_cuid_"), (re.compile(r"(\.L|\b)BB\d+_"), r"\1BB_"),
              (re.compile(r"\.Lfunc_(begin|end)\d+"), r".Lfunc_\1"), (re.compile(r"\.LJTI\d+_"), ".LJTI_"),
              (re.compile(r"^(\.LBB_\d+:)\s+;"), r"\1 ;"))  # (the comment column moves when the function index gains a digit)


def functions(asm: str):
    """{mangled name: normalised text} of every function, and the set of names that are kernels."""
    out, kernels, name, lines = {}, set(), None, []
    for line in asm.splitlines():
        m = re.search(r"; -- Begin function (\S+)", line)
        if m:
            name, lines = m.group(1), []
        if name is not None:
            for rx, to in _NORMALISE:
                line = rx.sub(to, line)
            lines.append(line)
            k = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
            if k:
                kernels.add(k.group(1))
            if "; -- End function" in line:
                out[name] = "\n".join(lines)
                name = None
    return out, kernels


def resources(remarks: str):
    """{function name: {field: value}} of the kernel-resource-usage remarks."""
    out, cur = {}, None
    for line in remarks.splitlines():
        m = re.search(r"remark:\s+(.*?)\s*\[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        key, _, val = m.group(1).partition(":")
        if key.strip() == "Function Name":
            cur = out.setdefault(val.strip(), {})
        elif cur is not None:
            cur[key.strip()] = val.strip()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--keep", help="directory for the assembly and remark files (default: a temporary one)")
    args = ap.parse_args()
    tmp = None
    if args.keep:
        work = pathlib.Path(args.keep)
        work.mkdir(parents=True, exist_ok=True)
    else:
        tmp = tempfile.TemporaryDirectory()
        work = pathlib.Path(tmp.name)
    with cf.ThreadPoolExecutor(max_workers=max(1, args.jobs)) as pool:
        jobs = {(side, u): pool.submit(compile_unit, tree, u, str(work / f"{side}_{u}.s"))
                for side, tree in (("a", args.tree_a), ("b", args.tree_b)) for u in UNITS}
        files = {k: f.result() for k, f in jobs.items()}
    bad = 0
    for u in UNITS:
        fa, ka = functions(pathlib.Path(files["a", u]).read_text())
        fb, kb = functions(pathlib.Path(files["b", u]).read_text())
        ra, rb = (resources(pathlib.Path(files[s, u] + ".remarks").read_text()) for s in ("a", "b"))
        only = sorted(set(fa) ^ set(fb))
        text = sorted(n for n in set(fa) & set(fb) if fa[n] != fb[n])
        res = sorted(n for n in set(ra) | set(rb) if ra.get(n) != rb.get(n))
        print(f"{u}: {len(ka)} / {len(kb)} kernels, {len(fa)} / {len(fb)} functions, {len(ra)} / {len(rb)} with resource remarks; "
              f"{len(only)} in one tree only, {len(text)} differ in text, {len(res)} differ in resources")
        for label, names in (("only in one tree", only), ("text differs", text), ("resources differ", res)):
            for n in names:
                print(f"  {label}: {n}")
        bad += len(only) + len(text) + len(res) + (ka != kb)
    if tmp:
        tmp.cleanup()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
