#!/usr/bin/env python3
"""Throughput of reverse complement: the one-shot call against the stream.

Image: one C4-shaped metagenome, 2M x 150-base records at 70 columns
(tests/synth.to_fasta), about 350 MB, generated once from a seed.

What is timed (wall clock around calls that return after the last byte has
reached the host, so every figure holds the upload, the kernels, the download
and the host copy into the caller's buffer):
  oneshot   imsame_dev_revcomp into a preallocated buffer
  stream W  imsame_dev_revcomp_stream with window W, the sink copying into a
            preallocated buffer (64 MiB, 256 MiB, 1 GiB)
  tool      imsame_amd/bin/revComp IN OUT, the whole process, on a file

Two libraries are compared in ONE session, alternating: --parent-lib names a
build of the parent commit's libimsame_dev.so (it has the one-shot call only)
and the package's own library is the new one.  Every measurement runs in a
child process that loads one library (one process on the GPU at a time), does
one warm-up call and one timed call; the parent alternates parent / new for
--rounds rounds, so both see the same machine.  The children also hash their
output: all must agree.

--avav LABEL=PATH (repeatable) runs that imsame_all_vs_all binary on the
all-vs-all golden and reports the revcomp= phase of its stderr line.

Prints one JSON object; writes nothing else.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
WINDOWS = {"64MiB": 64 << 20, "256MiB": 256 << 20, "1GiB": 1 << 30}


def make_image(path, records):
    import numpy as np                                           # noqa: F401
    from tests import synth
    ref, rst = synth.make_reference_arr(records * 150, 150, seed=41)
    with open(path, "wb") as f:
        f.write(synth.to_fasta(ref, rst, "m", width=70))


def child(args):
    """one library, one mode: warm-up + one timed call; prints a JSON line"""
    import numpy as np
    import imsame_amd                            # (sets the hardware-queue default as every Python host does)
    from imsame_amd import abi
    data = np.fromfile(args.image, dtype=np.uint8)
    # the library straight through ctypes: the parent's build has no stream
    # entry point, which the package's own binding asks for
    L = C.CDLL(imsame_amd.LIB_DEV)
    vp, u64 = C.c_void_p, C.c_uint64
    L.imsame_dev_open.argtypes = [C.c_int, C.POINTER(vp)]
    L.imsame_dev_close.argtypes = [vp]
    L.imsame_dev_revcomp.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64)]
    cap = len(data) + len(data) // 32 + 4096
    out = np.zeros(cap, dtype=np.uint8)
    ol = C.c_uint64()
    h = vp()
    assert L.imsame_dev_open(0, C.byref(h)) == 0
    try:
        if args.child == "oneshot":
            def call():
                rc = L.imsame_dev_revcomp(h, data.ctypes.data, len(data), out.ctypes.data, cap, C.byref(ol))
                assert rc == 0, rc
        else:
            window = int(args.child)
            at = [0]

            def src(_u, off, n, dst):
                C.memmove(dst, data.ctypes.data + off, n)
                return 0

            def snk(_u, p, n):
                C.memmove(out.ctypes.data + at[0], p, n)
                at[0] += n
                return 0
            s_fn, k_fn = abi.RC_SOURCE_FN(src), abi.RC_SINK_FN(snk)
            abi.bind_revcomp_stream(L)

            def call():
                at[0] = 0
                rc = L.imsame_dev_revcomp_stream(h, s_fn, None, len(data), window, k_fn, None, C.byref(ol))
                assert rc == 0, rc
        call()
        t = time.perf_counter()
        call()
        dt = time.perf_counter() - t
    finally:
        L.imsame_dev_close(h)
    print(json.dumps({"s": dt, "bytes_in": len(data), "bytes_out": ol.value,
                      "sha1": hashlib.sha1(out[:ol.value]).hexdigest()}))


def run_child(image, mode, lib=None):
    env = dict(os.environ)
    if lib:
        env["IMSAME_LIB_DEV"] = lib
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--image", image, "--child", mode], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    if p.returncode:
        raise SystemExit(f"child {mode} ({lib or 'new'}) failed ({p.returncode}):\n{p.stderr[-2000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def summary(xs):
    return {"median_s": statistics.median(xs), "min_s": min(xs), "max_s": max(xs), "runs_s": [round(x, 4) for x in xs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=2_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", help="libimsame_dev.so built from the parent commit")
    ap.add_argument("--workdir", help="where the image and the tool's output go (default: a temporary directory)")
    ap.add_argument("--avav", action="append", default=[], metavar="LABEL=PATH")
    ap.add_argument("--image")
    ap.add_argument("--child")
    args = ap.parse_args()
    if args.child:
        return child(args)

    work = args.workdir or tempfile.mkdtemp(prefix="bench_revcomp_")
    os.makedirs(work, exist_ok=True)
    image = os.path.join(work, f"c4_{args.records}.fa")
    if not os.path.exists(image):
        make_image(image, args.records)
    times, sha = {}, set()
    modes = [("new_oneshot", "oneshot", None)] + [(f"new_stream_{k}", str(w), None) for k, w in WINDOWS.items()]
    if args.parent_lib:
        modes.insert(0, ("parent_oneshot", "oneshot", os.path.abspath(args.parent_lib)))
    size = None
    for _ in range(args.rounds):                 # alternate: every mode once per round
        for label, mode, lib in modes:
            r = run_child(image, mode, lib)
            times.setdefault(label, []).append(r["s"])
            sha.add(r["sha1"])
            size = (r["bytes_in"], r["bytes_out"])
    from imsame_amd import REVCOMP
    outp = os.path.join(work, "tool.out")
    for _ in range(args.rounds):
        t = time.perf_counter()
        subprocess.run([REVCOMP, image, outp], check=True, timeout=600)
        times.setdefault("tool_end_to_end", []).append(time.perf_counter() - t)
    with open(outp, "rb") as f:
        h = hashlib.sha1()
        for blk in iter(lambda: f.read(1 << 24), b""):
            h.update(blk)
    sha.add(h.hexdigest())
    res = {"image": {"records": args.records, "bytes_in": size[0], "bytes_out": size[1]},
           "outputs_agree": len(sha) == 1, "rounds": args.rounds}
    for label, xs in times.items():
        res[label] = summary(xs)
        res[label]["GB_per_s_in"] = size[0] / statistics.median(xs) / 1e9

    gold = os.path.join(REPO, "tests", "golden", "avav")
    meta = json.load(open(os.path.join(gold, "expected.json"))) if args.avav else None
    for spec in args.avav:
        label, path = spec.split("=", 1)
        vals = []
        for _ in range(args.rounds):
            d = tempfile.mkdtemp(prefix="bench_avav_")
            try:
                shutil.copytree(os.path.join(gold, "in"), os.path.join(d, "m"))
                os.makedirs(os.path.join(d, "o"))
                p = subprocess.run([os.path.abspath(path), os.path.join(d, "m"), meta["cov"], meta["sim"], "1", "fa",
                                    os.path.join(d, "o")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                                   timeout=300, check=True)
                line = [ln for ln in p.stderr.splitlines() if " phase " in ln][-1]
                vals.append(float(line.split("revcomp=")[1].split()[0]))
            finally:
                shutil.rmtree(d, ignore_errors=True)
        res[f"avav_revcomp_phase_{label}"] = summary(vals)
    if not args.workdir:
        shutil.rmtree(work, ignore_errors=True)
    print(json.dumps(res))
    if not res["outputs_agree"]:
        raise SystemExit("outputs differ between the measured paths")


if __name__ == "__main__":
    main()
