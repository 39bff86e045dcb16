"""Developer timing of gzip pseudoalignment input: the strands inflated on the device (inflate_kernels.hpp behind
msw_alignment_read_device) against zlib on the host behind the same call (MSWEEP_HOST_INFLATE=1), on the same box in the
same process, with the plain-text pair as the floor.  Workload: the two Themisto strands of `reads` reads x `groups`
groups as `bench.py --config e2e` writes them (cfg3: 10 000 000 x 5 000, the default), gzip at level 6.
  - msw_alignment_read_device alone, and text -> abundances.txt (read, likelihood build, solve to 1e-6, the file), per
    side: plain, device inflate at the default chunk size, at 32 KiB and at 128 KiB, host inflate; the sides alternate
    inside every repeat, `reps` repeats after one unmeasured pass that warms the page cache for all of them
    (min / median / max);
  - the stage times of the device side from msw_inflate_info (upload on the host clock; probe, pass (a) + scan, window
    chain, pass (b), CRC from events on the reader's stream), median over the repeats, per strand;
  - the verdict the default rests on: the device side's median against the host side's, beside the spread of both.
With --bgzf the same strands are also written as BGZF (bgzip's blocked gzip: level 6, members of 0xff00 bytes of text,
htslib's end-of-file marker), which the member kernel inflates (inflate_member_kernels.hpp), and the sides are: the plain
pair (the floor), the BGZF pair on the device, the same BGZF pair with MSWEEP_HOST_INFLATE=1 -- what a build without the
member path does with these files -- and the single-member gzip pair on the device, for context.  --parent-lib PATH then
times the BGZF pair once more in a fresh process under MSWEEP_CORE_LIB=PATH (a library built from the commit before the
member path), as it is: no switch set.
usage: python tools/inflate_timing.py [reads] [groups] [reps] [--bgzf] [--parent-lib PATH]
       (MSWEEP_PROBE_DIR keeps the generated strands; MSWEEP_TEXT_TMPFS: where they go, /dev/shm by default)"""
import io, os, shutil, struct, subprocess, sys, tempfile, time, zlib
from concurrent.futures import ThreadPoolExecutor
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from msweep_amd import synth
from msweep_amd.core import Core
from msweep_amd.likelihood import from_device_alignment
from msweep_amd.sample import PlainSample

ARGS = list(sys.argv[1:])
BGZF = "--bgzf" in ARGS
CHILD = "--child" in ARGS          # (internal: the fresh process of --parent-lib; the strands and meta.npz are in MSWEEP_PROBE_DIR)
PARENT_LIB = ARGS[ARGS.index("--parent-lib") + 1] if "--parent-lib" in ARGS else None
NUMS = [a for a in ARGS if a.isdigit()]
R = int(NUMS[0]) if len(NUMS) > 0 else 10_000_000
G = int(NUMS[1]) if len(NUMS) > 1 else 5000
REPS = int(NUMS[2]) if len(NUMS) > 2 else 5


def stats(ts):
    ts = sorted(ts)
    return f"min {ts[0]:.3f} s, median {ts[len(ts) // 2]:.3f} s, max {ts[-1]:.3f} s"


def median(ts):
    return sorted(ts)[len(ts) // 2]


def gzip_file(src, dst, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, 31)
    with open(src, "rb") as f, open(dst, "wb") as g:
        while True:
            b = f.read(1 << 24)
            if not b:
                break
            g.write(c.compress(b))
        g.write(c.flush())


def bgzf_member(piece):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    payload = c.compress(piece) + c.flush()
    return (bytes.fromhex("1f8b08040000000000ff060042430200") + struct.pack("<H", len(payload) + 25) + payload +
            struct.pack("<II", zlib.crc32(piece), len(piece)))


def bgzf_file(src, dst, piece=0xff00):
    """src as BGZF: members of `piece` bytes of text, the end-of-file marker behind them (zlib releases the GIL: a
    thread per CPU the job may use)"""
    with open(src, "rb") as f, open(dst, "wb") as g, ThreadPoolExecutor(int(os.environ.get("OMP_NUM_THREADS", "16"))) as pool:
        while True:
            b = f.read(piece * 4096)
            if not b:
                break
            g.write(b"".join(pool.map(bgzf_member, [b[o:o + piece] for o in range(0, len(b), piece)])))
        g.write(bgzf_member(b""))


keep = os.environ.get("MSWEEP_PROBE_DIR")
tmp = keep or tempfile.mkdtemp(prefix="msweep_inflate_", dir=os.environ.get("MSWEEP_TEXT_TMPFS", "/dev/shm"))
os.makedirs(tmp, exist_ok=True)
try:
    plain = [os.path.join(tmp, f"reads_{k + 1}.txt") for k in range(2)]
    gz = [p + ".gz" for p in plain]
    blocked = [p + ".bgzf.gz" for p in plain]
    names = [f"g{g}" for g in range(G)]
    if CHILD:
        meta = np.load(os.path.join(tmp, "meta.npz"))
        n_targets, target_group, sizes = int(meta["n_targets"]), meta["target_group"], meta["sizes"]
    else:
        t0 = time.time()
        prob = synth.make_csr_problem(R, G, seed=1)
        aln = synth.csr_to_targets(prob, shuffle=False)
        E = len(prob["ec_counts"])
        rng = np.random.default_rng(11)
        ec_of = rng.permutation(np.repeat(np.arange(E, dtype=np.int64), prob["ec_counts"].astype(np.int64)))
        for k, path in enumerate(plain):
            synth.write_themisto(path, ec_of, aln["ec_tptr"], aln["ec_targets"], chunk=1_000_000,
                                 extra=(rng, 0.1, aln["n_targets"]) if k else None)
            gzip_file(path, gz[k])
            if BGZF:
                bgzf_file(path, blocked[k])
        n_targets, target_group, sizes = int(aln["n_targets"]), aln["target_group"], prob["group_sizes"]
        if PARENT_LIB:
            np.savez(os.path.join(tmp, "meta.npz"), n_targets=n_targets, target_group=target_group, sizes=sizes)
        del aln, ec_of
        mb = lambda ps: sum(os.path.getsize(p) for p in ps) / 1e6
        print(f"R={R} G={G}: two strands, {mb(plain):.1f} MB of text, {mb(gz):.1f} MB as gzip level 6 (ratio {mb(gz) / mb(plain):.3f})"
              + (f", {mb(blocked):.1f} MB as BGZF level 6 (ratio {mb(blocked) / mb(plain):.3f})" if BGZF else "") +
              f"; generated in {time.time() - t0:.0f} s; {REPS} repeats, sides alternated", flush=True)

    sides = {"plain": (plain, {}), "device": (gz, {}), "device-32K": (gz, {"MSWEEP_INFLATE_CHUNK": "32768"}),
             "device-128K": (gz, {"MSWEEP_INFLATE_CHUNK": "131072"}), "host": (gz, {"MSWEEP_HOST_INFLATE": "1"})}
    if BGZF:   # (the verdict below compares "device" with "host": here, the BGZF pair on both)
        sides = {"plain": (plain, {}), "device": (blocked, {}), "host": (blocked, {"MSWEEP_HOST_INFLATE": "1"}), "device-gzip": (gz, {})}
    if CHILD:  # the BGZF pair as the library given serves it
        sides = {"plain": (plain, {}), "as-is": (blocked, {})}
    read_s = {s: [] for s in sides}
    total_s = {s: [] for s in sides}
    infos = {s: [] for s in sides}
    texts = {}
    with Core(0) as core:
        core.set_pack_schedule(False)
        for rep in range(-1, REPS):   # (-1: unmeasured; page cache, allocator and clocks warm for every side)
            for side, (files, env) in sides.items():
                for k in ("MSWEEP_INFLATE_CHUNK", "MSWEEP_HOST_INFLATE"):
                    os.environ.pop(k, None)
                os.environ.update(env)
                t1 = time.perf_counter()
                al = core.read_alignment(files, n_targets, "intersection")
                t2 = time.perf_counter()
                lik = from_device_alignment(core, al, target_group, sizes)
                res = core.solve(None, np.ones(lik.n_groups))
                out = io.StringIO()
                smp = PlainSample(al.n_reads, al.n_aligned)
                smp.store_abundances(res["theta"])
                smp.write_abundances(names, out)
                with open(os.path.join(tmp, "abundances.txt"), "w") as f:
                    f.write(out.getvalue())
                t3 = time.perf_counter()
                assert al.on_device
                inf = core.last_inflate()
                want_dev = 1 if side.startswith("device") else 0
                assert CHILD or [i["on_device"] for i in inf] == [want_dev, want_dev], (side, inf)
                texts[side] = out.getvalue()
                if rep >= 0:
                    read_s[side].append(t2 - t1)
                    total_s[side].append(t3 - t1)
                    infos[side].append(inf)
                del al, lik
    assert all(t == texts["plain"] for t in texts.values()), "abundances.txt differs between the sides"
    print("msw_alignment_read_device (both strands, intersection):")
    for s in sides:
        print(f"  {s:12s} {stats(read_s[s])}")
    print("text -> abundances.txt (read, likelihood build, solve to 1e-6, the file; the same file on every side):")
    for s in sides:
        print(f"  {s:12s} {stats(total_s[s])}")
    if CHILD:
        print("  as-is: served by " + ", ".join("the device" if i["on_device"] else f"the host ({i['reason']})" for i in infos["as-is"][0]))
    for s in sides:
        if not s.startswith("device"):
            continue
        for k in range(2):
            if infos[s][0][k]["n_members"]:
                med = {key: median([rep[k][key] for rep in infos[s]]) for key in ("upload_ms", "write_ms", "kernel_ms")}
                i0 = infos[s][0][k]
                print(f"  {s:12s} strand {k + 1}: {i0['payload_bytes'] / 1e6:.1f} MB -> {i0['text_bytes'] / 1e6:.1f} MB in {i0['n_members']} members; "
                      f"median ms: upload (with the walk) {med['upload_ms']:.1f}, decode + trailer check {med['write_ms']:.1f} "
                      f"= {i0['text_bytes'] / (med['write_ms'] * 1e-3) / 1e9:.2f} GB/s of text")
                continue
            med = {key: median([rep[k][key] for rep in infos[s]]) for key in ("upload_ms", "probe_ms", "window_ms", "chain_ms", "write_ms", "crc_ms", "kernel_ms")}
            i0 = infos[s][0][k]
            print(f"  {s:12s} strand {k + 1}: {i0['payload_bytes'] / 1e6:.1f} MB -> {i0['text_bytes'] / 1e6:.1f} MB, chunk {i0['chunk_bytes']}, "
                  f"{i0['n_starts']} of {i0['n_chunks']} chunks begin an owner; median ms: upload {med['upload_ms']:.1f}, probe {med['probe_ms']:.1f}, "
                  f"pass a {med['window_ms']:.1f}, chain {med['chain_ms']:.1f}, pass b {med['write_ms']:.1f}, crc {med['crc_ms']:.1f}, "
                  f"kernels {med['kernel_ms']:.1f} = {i0['text_bytes'] / (med['kernel_ms'] * 1e-3) / 1e9:.2f} GB/s of text")
    for what, t in (() if CHILD else (("read", read_s), ("text -> abundances.txt", total_s))):
        d, h = median(t["device"]), median(t["host"])
        spread = max(max(t["device"]) - min(t["device"]), max(t["host"]) - min(t["host"]))
        print(f"{what}: device inflate median {d:.3f} s, host inflate median {h:.3f} s, largest spread of the repeats {spread:.3f} s: "
              f"{h / d:.2f} x ({'beats the host path by more than the spread' if h - d > spread else 'does NOT beat the host path by more than the spread'}); "
              f"plain text {median(t['plain']):.3f} s")
    if PARENT_LIB and not CHILD:
        print(f"the BGZF pair through the library of the commit before the member path ({REPS} repeats, a fresh process):\nlibrary: {PARENT_LIB}", flush=True)
        env = dict(os.environ, MSWEEP_CORE_LIB=os.path.abspath(PARENT_LIB), MSWEEP_PROBE_DIR=tmp)
        for k in ("MSWEEP_INFLATE_CHUNK", "MSWEEP_HOST_INFLATE"):
            env.pop(k, None)
        subprocess.check_call([sys.executable, os.path.abspath(__file__), str(R), str(G), str(REPS), "--bgzf", "--child"], env=env)
finally:
    if not keep and not CHILD:
        shutil.rmtree(tmp, ignore_errors=True)
