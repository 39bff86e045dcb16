"""Developer timing of --extract-reads (msw_fastq_*, fastq_kernels.hpp) against the second tool's method behind the same
calls (MSWEEP_HOST_EXTRACT=1 with MSWEEP_HOST_GZIP=1: zlib in, host gather, zlib out).  Themisto strands of `reads` reads x
`groups` groups (synth.write_themisto, as tools/bin_timing.py writes them) and two synthetic FASTQ files of `reads` records
x 150 bases, as single-member gzip level 6 and as BGZF; both sides alternated, medians of `reps` repeats, page cache warm:
  - open, split into upload (inflate included), the inflate kernels and the index, per form and side;
  - the bins with every group a target (thresholds 1 - theta) and the load case tools/bin_timing.py uses (thresholds
    0.5), selected and gathered target by target in pieces of 256 MiB: wall time of select + pieces, plain and inside a
    gzip stream, and the gather's GB/s of output from msw_fastq_last_timing;
  - msweep_mini as a whole process with --bin-reads --extract-reads, plain and --compress z, against the same run without
    --extract-reads.
usage: python tools/extract_timing.py [reads] [groups] [reps]   (MSWEEP_PROBE_DIR keeps the generated files)"""
import os, shutil, struct, subprocess, sys, tempfile, time, zlib
from concurrent.futures import ThreadPoolExecutor
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
G = int(sys.argv[2]) if len(sys.argv) > 2 else 5000
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 5
PIECE = 256 << 20
WORKERS = min(16, len(os.sched_getaffinity(0)))


def fastq_bytes(n, mate, seed):
    """n records of 150 bases with names of one width: one (n x record) byte matrix filled by columns"""
    rng = np.random.default_rng(seed)
    head = np.frombuffer(b"@read000000000/%d\n" % mate, np.uint8)
    w = len(head) + 151 + 2 + 151
    m = np.empty((n, w), np.uint8)
    m[:, :len(head)] = head
    ids = np.arange(n, dtype=np.int64)
    for d in range(9):
        m[:, 5 + 8 - d] = 48 + (ids // 10 ** d) % 10
    o = len(head)
    m[:, o:o + 150] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (n, 150), dtype=np.uint8)]
    m[:, o + 150] = 10
    m[:, o + 151] = 43
    m[:, o + 152] = 10
    m[:, o + 153:o + 303] = rng.integers(33, 74, (n, 150), dtype=np.uint8)
    m[:, o + 303] = 10
    return m.tobytes()


def _member(piece):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = c.compress(piece) + c.flush()
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(body) + 25) + body +
            struct.pack("<II", zlib.crc32(piece), len(piece)))


def _chunk(args):
    piece, last = args
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    return c.compress(piece) + (c.flush() if last else c.flush(zlib.Z_SYNC_FLUSH))


def write_forms(text, gz_path, bgzf_path):
    """single-member gzip level 6 (chunks of 8 MB compressed side by side and joined at sync flushes, as pigz joins them)
    and BGZF (members of 0xff00 bytes)"""
    with ThreadPoolExecutor(WORKERS) as ex:      # (zlib releases the interpreter lock)
        step = 8 << 20
        pieces = [(text[o:o + step], o + step >= len(text)) for o in range(0, len(text), step)]
        with open(gz_path, "wb") as f:
            f.write(b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff")
            for z in ex.map(_chunk, pieces):
                f.write(z)
            f.write(struct.pack("<II", zlib.crc32(text), len(text) & 0xffffffff))
        with open(bgzf_path, "wb") as f:
            for z in ex.map(_member, [text[o:o + 0xff00] for o in range(0, len(text), 0xff00)]):
                f.write(z)
            f.write(_member(b""))


def median(xs):
    return float(np.median(xs))


keep = os.environ.get("MSWEEP_PROBE_DIR")
tmp = keep or tempfile.mkdtemp(prefix="msweep_extract_", dir=os.environ.get("TMPDIR", "/tmp"))
os.makedirs(tmp, exist_ok=True)
try:
    from msweep_amd import binning, synth
    strands = [os.path.join(tmp, "r1.txt"), os.path.join(tmp, "r2.txt")]
    clus = os.path.join(tmp, "clustering.txt")
    t = time.perf_counter()
    if not (os.path.exists(clus) and all(os.path.exists(x) for x in strands)):
        prob = synth.make_csr_problem(R, G, seed=2)
        aln = synth.csr_to_targets(prob, shuffle=False)
        E = len(prob["ec_counts"])
        rng = np.random.default_rng(11)
        ec_of = rng.permutation(np.repeat(np.arange(E, dtype=np.int64), prob["ec_counts"].astype(np.int64)))
        for k, path in enumerate(strands):
            synth.write_themisto(path, ec_of, aln["ec_tptr"], aln["ec_targets"], chunk=1_000_000,
                                 extra=(rng, 0.1, aln["n_targets"]) if k else None)
        with open(clus, "w") as c:
            c.write("\n".join(f"g{int(g)}" for g in aln["target_group"]) + "\n")
        del prob, aln, ec_of
    forms = {"gzip": [os.path.join(tmp, f"reads_{k}.fq.gz") for k in (1, 2)],
             "bgzf": [os.path.join(tmp, f"reads_{k}.bgzf.fq.gz") for k in (1, 2)]}
    text_bytes = 0
    for k in (1, 2):
        if not (os.path.exists(forms["gzip"][k - 1]) and os.path.exists(forms["bgzf"][k - 1])):
            text = fastq_bytes(R, k, 40 + k)
            text_bytes = len(text)
            write_forms(text, forms["gzip"][k - 1], forms["bgzf"][k - 1])
            del text
    print(f"inputs generated in {time.perf_counter() - t:.1f} s: {R} reads x {G} groups; per FASTQ file {text_bytes / 1e6:.0f} MB of text, "
          f"{os.path.getsize(forms['gzip'][0]) / 1e6:.0f} MB as gzip, {os.path.getsize(forms['bgzf'][0]) / 1e6:.0f} MB as BGZF", flush=True)

    from msweep_amd.core import Core
    from msweep_amd.reference import read_reference
    grouping = read_reference(open(clus))
    sides = {"device": {"MSWEEP_HOST_EXTRACT": "0", "MSWEEP_HOST_GZIP": "0"}, "host": {"MSWEEP_HOST_EXTRACT": "1", "MSWEEP_HOST_GZIP": "1"}}
    with Core(0) as core:
        a = core.read_alignment(strands, len(grouping.group_indicators))
        kept, mask, _ = core.build_likelihood_aln(a, grouping.group_indicators, grouping.get_sizes(), want_logc=False)
        theta = core.solve(None, np.ones(kept))["theta"]
        rows = np.arange(kept, dtype=np.uint32)
        bins = {"1 - theta": core.bin_reads_aln(a, rows, binning.thresholds(rows, theta))[:2],
                "t = 0.5": core.bin_reads_aln(a, rows, np.full(kept, 0.5))[:2]}
        for name, (bp, ids) in bins.items():
            print(f"bins, thresholds {name}: {kept} targets, {int(bp[-1])} read ids", flush=True)

        # ---- open: upload (inflate included), inflate kernels, index ----
        for form, paths in forms.items():
            rec = {s: [] for s in sides}
            for _ in range(REPS):
                for side, env in sides.items():
                    os.environ.update(env)
                    t0 = time.perf_counter()
                    with core.fastq_open(paths[0]) as fq:
                        info = fq.info
                    rec[side].append((time.perf_counter() - t0, info["upload_ms"], info["inflate"]["kernel_ms"], info["index_ms"],
                                      info["inflate"]["on_device"], info["text_bytes"]))
            for side in sides:
                v = np.array(rec[side])
                print(f"open {form:5s} {side:6s}: {median(v[:, 0]) * 1e3:9.1f} ms (spread {(v[:, 0].max() - v[:, 0].min()) * 1e3:.1f}); upload with "
                      f"inflate {median(v[:, 1]):9.1f} ms, inflate kernels {median(v[:, 2]):8.1f} ms, index {median(v[:, 3]):8.1f} ms; "
                      f"inflated on the device: {int(v[0, 4])}; {v[0, 5] / 1e6:.0f} MB of text", flush=True)

        # ---- select + gather per target, plain and inside a gzip stream ----
        for name, (bp, ids) in bins.items():
            rec = {(s, z): [] for s in sides for z in (False, True)}
            for rep in range(REPS):
                for side, env in sides.items():
                    os.environ.update(env)
                    with core.fastq_open(forms["bgzf"][0]) as fq:
                        for z in (False, True):
                            t0 = time.perf_counter()
                            ms = nb = nz = 0
                            for k in range(kept):
                                fq.select(ids[int(bp[k]):int(bp[k + 1])])
                                if z:
                                    nz += len(core.gzip_begin(6)) + sum(len(p) for p in fq.pieces_gzip(PIECE)) + len(core.gzip_end())
                                else:
                                    nz += sum(len(p) for p in fq.pieces(PIECE))
                                tm = core.last_fastq_timing()
                                ms += tm[0]
                                nb += tm[1]
                            rec[(side, z)].append((time.perf_counter() - t0, ms, nb, nz))
            for (side, z), v in rec.items():
                v = np.array(v)
                gbs = v[0, 2] / 1e6 / max(median(v[:, 1]), 1e-9)
                print(f"extract {name:9s} {side:6s} {'gzip ' if z else 'plain'}: {median(v[:, 0]) * 1e3:9.1f} ms for {kept} selections, "
                      f"{v[0, 2] / 1e6:.1f} MB of records, {v[0, 3] / 1e6:.1f} MB out; gather {median(v[:, 1]):8.2f} ms = {gbs:6.1f} GB/s of output",
                      flush=True)
    for k in ("MSWEEP_HOST_EXTRACT", "MSWEEP_HOST_GZIP"):
        os.environ.pop(k, None)

    # ---- msweep_mini as a whole process ----
    exe = os.path.join(tmp, "msweep_mini")
    lib = os.path.join(ROOT, "msweep_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-o", exe, os.path.join(lib, "cpp", "msweep_mini.cpp"),
                           "-L" + lib, "-lmsweep_core", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    base = [exe, "--themisto-1", strands[0], "--themisto-2", strands[1], "-i", clus, "--bin-reads"]
    runs = {}
    for form, paths in forms.items():
        for z in (False, True):
            for side in sides:
                runs[(form, z, side)] = ["--extract-reads", ",".join(paths)] + (["--compress", "z"] if z else [])
    for z in (False, True):
        runs[("none", z, "device")] = ["--compress", "z"] if z else []
    times = {k: [] for k in runs}
    for rep in range(REPS):
        for key, extra in runs.items():
            out = os.path.join(tmp, "out")
            shutil.rmtree(out, ignore_errors=True)
            os.makedirs(out)
            env = dict(os.environ, **sides[key[2]])
            t0 = time.perf_counter()
            subprocess.run(base + extra + ["-o", os.path.join(out, "p")], check=True, env=env, capture_output=True)
            times[key].append(time.perf_counter() - t0)
            if rep == 0:
                nfq = [f for f in os.listdir(out) if ".fastq" in f]
                print(f"  ({key}: {len(nfq)} extraction files, {sum(os.path.getsize(os.path.join(out, f)) for f in nfq) / 1e6:.1f} MB)", flush=True)
    for key, v in times.items():
        print(f"msweep_mini --bin-reads, read files {key[0]:5s} {'--compress z' if key[1] else 'plain       '} {key[2]:6s}: "
              f"{median(v):7.3f} s (min {min(v):.3f}, max {max(v):.3f})", flush=True)
finally:
    if not keep:
        shutil.rmtree(tmp, ignore_errors=True)
