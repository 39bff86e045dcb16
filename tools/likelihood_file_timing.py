"""Developer timing of --read-likelihood: the file parsed on the device (likelihood_text_kernels.hpp behind
msw_core_set_dense_logl_file) against the drivers' own host parsers behind the same flag (MSWEEP_HOST_LIKELIHOOD_FILE=1),
on the same box, sides alternated inside every repeat.  Workload: the likelihood of `reads` reads x `groups` groups
(synth.make_csr_problem; about as many classes as reads), written by --write-likelihood's writer of this build, as plain
text, gzip level 6 and BGZF.
  - the entry alone (Core.set_dense_logl_file): wall time, and upload_ms / kernel_ms of msw_likfile_info as GB/s of text;
  - `msweep_mini --read-likelihood` as a whole process (--mini PATH: the binary built against this tree's library) and the
    Python driver in-process, each device against host (--no-python-host: without the Python host side, whose float()
    per cell takes minutes at 10^8 cells);
  - --parent-mini PATH: the msweep_mini of the parent commit, linked to the parent commit's library, on the plain file
    only (it cannot read the others).  The Python driver's host side IS the parent's code path.
The host side of a `.gz` file: the Python driver inflates with gzip.open; msweep_mini's host parser inflates through
msw_core_inflate_gzip, i.e. on the device unless MSWEEP_HOST_INFLATE=1 is set too -- its `.gz` host rows measure the host
PARSE behind a device inflate.  One shape per invocation; profiles/likelihood_file_timing.txt lists the invocations.
min / median / max of `reps` repeats after one unmeasured pass; the verdict compares medians beside the larger spread.
usage: python tools/likelihood_file_timing.py [reads] [groups] [reps] [--mini PATH] [--parent-mini PATH] [--no-python-host]
       (MSWEEP_TEXT_TMPFS: where the files go, /dev/shm by default)"""
import os, shutil, struct, subprocess, sys, tempfile, time, zlib
from concurrent.futures import ThreadPoolExecutor
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from msweep_amd import synth
from msweep_amd.__main__ import main, write_likelihood_file
from msweep_amd.core import Core
from msweep_amd.likelihood import from_grouped_counts

ARGS = list(sys.argv[1:])
opt = lambda name: ARGS[ARGS.index(name) + 1] if name in ARGS else None
MINI, PARENT_MINI, NO_PY_HOST = opt("--mini"), opt("--parent-mini"), "--no-python-host" in ARGS
NUMS = [a for a in ARGS if a.isdigit()]
R = int(NUMS[0]) if len(NUMS) > 0 else 100_000
G = int(NUMS[1]) if len(NUMS) > 1 else 1000
REPS = int(NUMS[2]) if len(NUMS) > 2 else 5
SWITCH = "MSWEEP_HOST_LIKELIHOOD_FILE"


def stats(ts):
    ts = sorted(ts)
    return f"min {ts[0]:.3f} s, median {ts[len(ts) // 2]:.3f} s, max {ts[-1]:.3f} s"


def median(ts):
    return sorted(ts)[len(ts) // 2]


def bgzf_member(piece):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    payload = c.compress(piece) + c.flush()
    return (bytes.fromhex("1f8b08040000000000ff060042430200") + struct.pack("<H", len(payload) + 25) + payload +
            struct.pack("<II", zlib.crc32(piece), len(piece)))


def compress_files(src, gz, blocked, piece=0xff00):
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    with open(src, "rb") as f, open(gz, "wb") as g, open(blocked, "wb") as b, \
            ThreadPoolExecutor(int(os.environ.get("OMP_NUM_THREADS", "16"))) as pool:
        while True:
            d = f.read(piece * 1024)
            if not d:
                break
            g.write(c.compress(d))
            b.write(b"".join(pool.map(bgzf_member, [d[o:o + piece] for o in range(0, len(d), piece)])))
        g.write(c.flush())
        b.write(bgzf_member(b""))


tmp = tempfile.mkdtemp(prefix="msweep_likfile_", dir=os.environ.get("MSWEEP_TEXT_TMPFS", "/dev/shm"))
try:
    t0 = time.time()
    files = {"plain": os.path.join(tmp, "lik.tsv"), "gzip": os.path.join(tmp, "lik.tsv.gz"), "bgzf": os.path.join(tmp, "lik.bgzf.gz")}
    groups = os.path.join(tmp, "groups.txt")
    with open(groups, "w") as f:
        f.write("".join(f"g{g}\n" for g in range(G)))
    with Core(0) as core:
        prob = synth.make_csr_problem(R, G, seed=1)
        lik = from_grouped_counts(core, prob["rowptr"], prob["grp"], prob["cnt"], prob["ec_counts"], prob["group_sizes"])
        with open(files["plain"], "wb") as f:
            write_likelihood_file(f, prob["ec_counts"], lik)
        E = lik.n_ecs
    compress_files(files["plain"], files["gzip"], files["bgzf"])
    size = {k: os.path.getsize(p) for k, p in files.items()}
    print(f"E={E} G={G}: {size['plain'] / 1e6:.1f} MB of likelihood text, {size['gzip'] / 1e6:.1f} MB as gzip level 6, "
          f"{size['bgzf'] / 1e6:.1f} MB as BGZF; written in {time.time() - t0:.0f} s; {REPS} repeats, sides alternated", flush=True)

    def run_mini(binary, path, host):
        env = dict(os.environ)
        env.pop(SWITCH, None)
        if host:
            env[SWITCH] = "1"
        t1 = time.perf_counter()
        subprocess.run([binary, "-i", groups, "--read-likelihood", path, "-o", os.path.join(tmp, "mini")], check=True, env=env,
                       capture_output=True)
        dt = time.perf_counter() - t1
        return dt, open(os.path.join(tmp, "mini_abundances.txt")).read()

    def run_python(path, host):
        os.environ.pop(SWITCH, None)
        if host:
            os.environ[SWITCH] = "1"
        t1 = time.perf_counter()
        assert main(["-i", groups, "--read-likelihood", path, "-o", os.path.join(tmp, "py")]) == 0
        dt = time.perf_counter() - t1
        os.environ.pop(SWITCH, None)
        return dt, open(os.path.join(tmp, "py_abundances.txt")).read()

    sides = {}
    for fmt, path in files.items():
        sides[f"entry alone, {fmt}"] = ("entry", path, False)
        if MINI:
            sides[f"msweep_mini device, {fmt}"] = ("mini", path, False)
            sides[f"msweep_mini host, {fmt}"] = ("mini", path, True)
        sides[f"python device, {fmt}"] = ("python", path, False)
        if not NO_PY_HOST:
            sides[f"python host, {fmt}"] = ("python", path, True)
    if PARENT_MINI:
        sides["msweep_mini parent commit, plain"] = ("parent", files["plain"], False)
    times = {s: [] for s in sides}
    infos = {s: [] for s in sides}
    outs = {}
    with Core(0) as core:
        for rep in range(-1, REPS):      # (-1: unmeasured; page cache, allocator and clocks warm for every side)
            for side, (kind, path, host) in sides.items():
                if kind == "entry":
                    t1 = time.perf_counter()
                    info, counts = core.set_dense_logl_file(path, G)
                    dt = time.perf_counter() - t1
                    assert info["served"] == 1 and info["n_ecs"] == E, info
                    out = None
                elif kind == "python":
                    dt, out = run_python(path, host)
                else:
                    dt, out = run_mini(PARENT_MINI if kind == "parent" else MINI, path, host)
                if out is not None:
                    outs.setdefault(kind == "python", out)
                    assert out == outs[kind == "python"], f"abundances differ: {side}"
                if rep >= 0:
                    times[side].append(dt)
                    if kind == "entry":
                        infos[side].append(info)
    for s in sides:
        print(f"  {s:36s} {stats(times[s])}")
    for fmt in files:
        s = f"entry alone, {fmt}"
        up, ke = median([i["upload_ms"] for i in infos[s]]), median([i["kernel_ms"] for i in infos[s]])
        i0 = infos[s][0]
        print(f"  {s}: {i0['text_bytes'] / 1e6:.1f} MB of text, {i0['n_host_cells']} cells on the host; median ms: upload"
              f"{' + inflate' if fmt != 'plain' else ''} {up:.1f} = {i0['text_bytes'] / (up * 1e-3) / 1e9:.2f} GB/s, "
              f"parse + transpose {ke:.1f} = {i0['text_bytes'] / (ke * 1e-3) / 1e9:.2f} GB/s of text")

    def verdict(what, dev, base):
        if dev not in times or base not in times:
            return
        d, h = median(times[dev]), median(times[base])
        spread = max(max(times[dev]) - min(times[dev]), max(times[base]) - min(times[base]))
        word = "faster by more than the spread" if h - d > spread else ("SLOWER by more than the spread" if d - h > spread else "no difference beyond the spread")
        print(f"{what}: device median {d:.3f} s, {base} median {h:.3f} s, largest spread {spread:.3f} s: {h / d:.2f} x ({word})")

    for fmt in files:
        verdict(f"msweep_mini, {fmt}", f"msweep_mini device, {fmt}", f"msweep_mini host, {fmt}")
        verdict(f"python driver, {fmt}", f"python device, {fmt}", f"python host, {fmt}")
    verdict("msweep_mini against the parent commit, plain", "msweep_mini device, plain", "msweep_mini parent commit, plain")
finally:
    shutil.rmtree(tmp, ignore_errors=True)
