#!/usr/bin/env python3
"""End-to-end run of the CLI on the GPU box (SURVEY.md 8(d) "Mapped all reads" analogue):
synthetic genome + index built on the device and written to disk in the reference's formats,
synthetic read pairs written as FASTQ, then `chromap-amd --preset atac` from files to BED.
`--preset hic`: 2 x 150 Hi-C shaped pairs with ligation junctions (the generator of bench.py's hic workload), `chromap-amd --preset hic`
from files to a pairs file, through the device ingest (read names kept in HBM) and through the host parser (`--host-ingest`, the route
every pairs run took before), plain FASTQ and -- with --gz -- BGZF, `--reps` runs each; the pairs files must be identical.
`--sam`: 2 x 150 ordinary pairs, `chromap-amd --preset chip --SAM` from files to a SAM file through the device ingest (whole reads and
alignment records kept in HBM, text rendered there) and through the host parser and writer (`--host-ingest`), timed like the hic routes.
`--barcodes N`: a single-cell job -- a whitelist of N random 16-mers, every pair draws one, 10 % of them with one substitution (the
generator of tools/ref_baseline.py); `--summary` then times the same job without and with `--summary FILE`, `--reps` runs each, and
`--baseline-cli` the build of an earlier commit on the same files (without `--summary`; with `--gz` on the BGZF files too).
`--output-bgzf` (with `--preset hic` or `--sam`): the job plain, the job with `--output-bgzf` (BGZF blocks compressed on the device), and what
a user does without the flag -- the plain run followed by tools/bgzf.py on its output (zlib level 1, 16 threads); `--reps` runs each, whole-process
wall time, output sizes, and the compressed file inflated and compared with the plain one.  `--baseline-cli`: the plain job with that build too.
`--output-tbi` (with `--preset atac`, with or without `--barcodes`): the job with `--output-bgzf`, the job with `--output-bgzf --output-tbi`
(the tabix index built on the device) and -- with `--baseline-cli` -- that build with `--output-bgzf`; the builds and flags take turns,
`--reps` rounds, whole-process wall time; the outputs must inflate to the same text, and the index's own line is kept.
`--output-bam` (with `--sam`): the job as plain `--SAM`, as `--SAM --output-bgzf` and as `--BAM` (records encoded and compressed on the
device), `--reps` runs each, whole-process wall time and file sizes; the first records of the BAM file, decoded by tests/bam_model.py, must be
the first lines of the SAM file.
`--output-bai` (with `--sam`): the job as `--BAM` and as `--BAM --output-bai` (the BAM index built on the device) and -- with
`--baseline-cli` -- that build with `--BAM`; the builds and flags take turns, `--reps` rounds, whole-process wall time; the BAM files must
be the same bytes, and the index's own line is kept.  With `--output-csi` as well: a further run per round as `--BAM --output-csi` (the
CSI index built on the device), its own line and the `.csi` file's size kept beside the `.bai`'s.
Prints one JSON object; everything is written under --dir (default /tmp/chromap_amd_e2e)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from chromap_amd.cpus import cpu_budget  # noqa: E402


def write_fastq(path, bases, n, L):
    name = np.char.add("@r", np.char.zfill(np.arange(n).astype(str), 9)).astype("S11")
    rec = np.empty((n, 11 + 1 + L + 3 + L + 1), np.uint8)
    rec[:, :11] = np.frombuffer(name.tobytes(), np.uint8).reshape(n, 11)
    rec[:, 11] = 10
    rec[:, 12:12 + L] = bases.reshape(n, L)
    rec[:, 12 + L:15 + L] = np.frombuffer(b"\n+\n", np.uint8)
    rec[:, 15 + L:15 + 2 * L] = ord("I")
    rec[:, 15 + 2 * L] = 10
    rec.tofile(path)


def write_barcodes(d, n_all, n_wl, seed=1000):
    """whitelist.txt and bc.fq under d; returns the CLI's arguments for them"""
    rng = np.random.default_rng(seed)
    wl = np.unique(rng.integers(0, 1 << 32, size=n_wl, dtype=np.uint64))  # 16-mers as 32-bit codes
    acgt = np.frombuffer(b"ACGT", np.uint8)
    shifts = (2 * np.arange(15, -1, -1)).astype(np.uint64)

    def letters(codes):
        return acgt[((codes[:, None] >> shifts[None, :]) & np.uint64(3)).astype(np.int64)]
    wl_path, bc_path = os.path.join(d, "whitelist.txt"), os.path.join(d, "bc.fq")
    with open(wl_path, "wb") as f:
        f.write(b"\n".join(bytes(x) for x in letters(wl)) + b"\n")
    seq = letters(wl[rng.integers(0, len(wl), size=n_all)])
    rows = np.nonzero(rng.random(n_all) < 0.10)[0]
    seq[rows, rng.integers(0, 16, size=len(rows))] = acgt[rng.integers(0, 4, size=len(rows))]
    rec = np.empty((n_all, 39), np.uint8)  # "@b\n" + 16 + "\n+\n" + 16 x 'I' + "\n"
    rec[:, 0:3] = np.frombuffer(b"@b\n", np.uint8)
    rec[:, 3:19] = seq
    rec[:, 19:22] = np.frombuffer(b"\n+\n", np.uint8)
    rec[:, 22:38] = ord("I")
    rec[:, 38] = ord("\n")
    rec.tofile(bc_path)
    return ["-b", bc_path, "--barcode-whitelist", wl_path]


def output_tbi_job(args, cli, job, out):
    """--output-bgzf with the parent's build (--baseline-cli), with this build, and with this build and --output-tbi: one run of each per
    round, the order kept, after one untimed round"""
    import hashlib
    import zlib
    variants = ([("parent_output_bgzf", args.baseline_cli, ["--output-bgzf"])] if args.baseline_cli else []) + \
               [("output_bgzf", cli, ["--output-bgzf"]), ("output_bgzf_output_tbi", cli, ["--output-bgzf", "--output-tbi"])]
    res = {label: {"wall_s": [], "lines": []} for label, _, _ in variants}

    def md5_inflated(path):
        h = hashlib.md5()
        d = zlib.decompressobj(31)
        with open(path, "rb") as f:
            for b in iter(lambda: f.read(1 << 24), b""):
                while b:
                    h.update(d.decompress(b))
                    if d.eof:   # the next BGZF block
                        b = d.unused_data
                        d = zlib.decompressobj(31)
                    else:
                        b = b""
        return h.hexdigest()
    for rnd in range(args.reps + 1):
        for label, exe, extra in variants:
            for f in (out, out + ".tbi"):
                if os.path.exists(f):
                    os.remove(f)
            os.sync()
            t0 = time.time()
            p = subprocess.run([exe] + job + extra, stderr=subprocess.PIPE, check=True)
            dt = time.time() - t0
            if rnd == 0:   # untimed: every build's code objects and the files have been read once
                res[label]["text_md5"] = md5_inflated(out)
                res[label]["bgzf_bytes"] = os.path.getsize(out)
                if "--output-tbi" in extra:
                    res[label]["tbi_bytes"] = os.path.getsize(out + ".tbi")
                continue
            res[label]["wall_s"].append(round(dt, 3))
            res[label]["lines"].append([ln for ln in p.stderr.decode().splitlines()
                                        if ln.startswith(("Mapped all reads", "Sorted,", "Compressed ", "Built the tabix index", "Number of output mappings"))])
    res["same_text"] = len({res[label]["text_md5"] for label, _, _ in variants}) == 1
    res["config"] = {"pairs": args.pairs, "readlen": args.readlen, "genome": args.genome, "barcodes": args.barcodes, "reps": args.reps,
                     "hardware_threads": os.cpu_count(), "cpu_budget": cpu_budget()}
    return res


def output_bai_job(args, cli, job, out):
    """--BAM with the parent's build (--baseline-cli), with this build, and with this build and --output-bai: one run of each per round,
    the order kept, after one untimed round"""
    variants = ([("parent_bam", args.baseline_cli, ["--BAM"])] if args.baseline_cli else []) + \
               [("bam", cli, ["--BAM"]), ("bam_output_bai", cli, ["--BAM", "--output-bai"])] + \
               ([("bam_output_csi", cli, ["--BAM", "--output-csi"])] if args.output_csi else [])   # (--output-csi: the .csi beside the .bai, same session and build)
    res = {label: {"wall_s": [], "lines": []} for label, _, _ in variants}
    for rnd in range(args.reps + 1):
        for label, exe, extra in variants:
            for f in (out, out + ".bai", out + ".csi"):
                if os.path.exists(f):
                    os.remove(f)
            os.sync()
            t0 = time.time()
            p = subprocess.run([exe] + job + extra, stderr=subprocess.PIPE, check=True)
            dt = time.time() - t0
            if rnd == 0:   # untimed: every build's code objects and the files have been read once
                if "--output-csi" in extra:
                    res[label]["csi_bytes"] = os.path.getsize(out + ".csi")
                res[label]["bam_md5"] = subprocess.check_output(["md5sum", out]).split()[0].decode()
                res[label]["bam_bytes"] = os.path.getsize(out)
                res[label]["bai_written"] = os.path.exists(out + ".bai")
                if "--output-bai" in extra:
                    res[label]["bai_bytes"] = os.path.getsize(out + ".bai")
                continue
            res[label]["wall_s"].append(round(dt, 3))
            res[label]["lines"].append([ln for ln in p.stderr.decode().splitlines()
                                        if ln.startswith(("Mapped all reads", "Compressed ", "Built the BAM index", "Built the CSI index", "Number of output mappings"))])
    res["same_bam"] = len({res[label]["bam_md5"] for label, _, _ in variants}) == 1
    res["config"] = {"preset": args.preset, "pairs": args.pairs, "readlen": args.readlen, "genome": args.genome, "reps": args.reps,
                     "hardware_threads": os.cpu_count(), "cpu_budget": cpu_budget()}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=200_000_000)
    ap.add_argument("--nseq", type=int, default=8)
    ap.add_argument("--pairs", type=int, default=8_000_000)
    ap.add_argument("--preset", default="atac", choices=("atac", "hic"))
    ap.add_argument("--readlen", type=int, default=0, help="default: 50 (atac), 150 (hic)")
    ap.add_argument("--dir", default="/tmp/chromap_amd_e2e")
    ap.add_argument("--gz", action="store_true", help="also time gzip-compressed input (inflated on the host, one thread per file) and BGZF input (on the device)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--baseline-cli", default="", help="--preset hic: also time this other chromap-amd binary (a build of an earlier commit) on the same files")
    ap.add_argument("--sam", action="store_true", help="time --preset chip --SAM through the device route and the host route (and --baseline-cli)")
    ap.add_argument("--barcodes", type=int, default=0, help="--preset atac: a single-cell job with a whitelist of this many 16-mers (scATAC: 737280)")
    ap.add_argument("--summary", action="store_true", help="--preset atac: also time the job with --summary FILE (and --baseline-cli without it)")
    ap.add_argument("--output-bgzf", action="store_true", help="--preset hic / --sam: time the job plain, with --output-bgzf, and plain + tools/bgzf.py of the output")
    ap.add_argument("--output-tbi", action="store_true", help="--preset atac: time --output-bgzf without and with --output-tbi (and --baseline-cli with --output-bgzf), taking turns")
    ap.add_argument("--output-bam", action="store_true", help="--sam: time the job as --SAM, --SAM --output-bgzf and --BAM")
    ap.add_argument("--output-bai", action="store_true", help="--sam: time --BAM without and with --output-bai (and --baseline-cli with --BAM), taking turns")
    ap.add_argument("--output-csi", action="store_true", help="--sam --output-bai: a fourth run per round with --BAM --output-csi")
    ap.add_argument("--skip-host-ingest", action="store_true", help="a long job: leave the host parser's run out")
    args = ap.parse_args()
    os.makedirs(args.dir, exist_ok=True)
    if args.sam:
        args.preset = "chip"
    hic = args.preset == "hic"
    two_routes = hic or args.sam  # the same files through the device route and the host route, whole-process wall time
    if not args.readlen:
        args.readlen = 150 if two_routes else 50
    from chromap_amd import ChromapGPU
    g = ChromapGPU(synthetic=(args.genome, args.nseq, 4242), preset="atac" if args.sam else args.preset)
    idx = os.path.join(args.dir, "g.index")
    fa = os.path.join(args.dir, "g.fa")
    g.save_index(idx)
    nseq = C.c_uint32(0)
    g.L.cmgpu_reference_lengths(g.ctx, None, 0, C.byref(nseq))
    lens = (C.c_uint32 * nseq.value)()
    g.L.cmgpu_reference_lengths(g.ctx, lens, nseq.value, C.byref(nseq))
    with open(fa, "wb") as f:
        for i in range(nseq.value):
            buf = C.create_string_buffer(lens[i])
            assert g.L.cmgpu_export_reference(g.ctx, i, buf, lens[i]) == 0
            f.write(b">chr%d\n" % (i + 1))
            f.write(buf.raw[:lens[i]])
            f.write(b"\n")
    if hic:  # mates from independent loci, 35 % of the reads with a ligation junction, 0.1 % indels: bench.py's hic workload
        g.generate_resident(args.pairs, read_length=args.readlen, sub_rate=0.01, seed=99, indel_rate=0.001, hic=0.35)
    else:
        g.generate_resident(args.pairs, read_length=args.readlen, frag_min=30, frag_max=600, sub_rate=0.01, seed=99)
    b1, o1, b2, o2 = g.download_batch(args.pairs)
    r1 = os.path.join(args.dir, "r1.fq")
    r2 = os.path.join(args.dir, "r2.fq")
    write_fastq(r1, b1, args.pairs, args.readlen)
    write_fastq(r2, b2, args.pairs, args.readlen)
    g.close()
    out = os.path.join(args.dir, "out.sam" if args.sam else "out.pairs" if hic else "out.bed")
    fmt = ["--SAM"] if args.sam else []
    cli = os.path.join(ROOT, "chromap_amd", "chromap-amd")
    res = {}
    job = write_barcodes(args.dir, args.pairs, args.barcodes) if args.barcodes else []

    if args.output_tbi:
        print(json.dumps(output_tbi_job(args, cli, ["--preset", args.preset, "-x", idx, "-r", fa, "-1", r1, "-2", r2, "-o", out + ".gz"] + job, out + ".gz")))
        return

    if args.output_bai and args.sam:
        print(json.dumps(output_bai_job(args, cli, ["--preset", args.preset, "-x", idx, "-r", fa, "-1", r1, "-2", r2, "-o", out + ".bam"] + job, out + ".bam")))
        return

    def run(label, f1, f2, extra=(), reps=args.reps, cli=cli, after=None):
        """the CLI `reps` times; the run with the shortest 'Mapped all reads' time is the one reported"""
        best = None
        times = []
        walls = []
        md5s_run = []
        for _ in range(reps):
            # every run starts from the same file-system state: no output file to truncate, no dirty pages of the run before
            # (the 246 MB a run writes are throttled by the write-back of the 246 MB the one before wrote)
            if os.path.exists(out):
                os.remove(out)
            os.sync()
            t0 = time.time()
            p = subprocess.run([cli, "--preset", args.preset, "-x", idx, "-r", fa, "-1", f1, "-2", f2, "-o", out] + fmt + job + list(extra), stderr=subprocess.PIPE, check=True)
            if after:  # (what follows the run belongs to the job's wall time)
                after()
            dt = time.time() - t0
            tail = [ln for ln in p.stderr.decode().splitlines() if ln.startswith("Mapped all reads") or ln.startswith("Sorted,") or ln.startswith("Compressed ")]
            mapped = [float(ln.split("in ")[1].split("s")[0]) for ln in tail if ln.startswith("Mapped all reads")]
            mapped = mapped[0] if mapped else None
            times.append(mapped)
            walls.append(round(dt, 3))
            md5s_run.append(subprocess.check_output(["md5sum", out]).split()[0].decode())
            # (the host parser's run prints no "Mapped all reads" line: its runs are ranked by wall time)
            if best is None or (mapped is not None and mapped < best["mapped_all_reads_s"]) or (mapped is None and dt < best["wall_s"]):
                best = {"wall_s": round(dt, 2), "M_pairs_per_s_wall": round(args.pairs / dt / 1e6, 2), "mapped_all_reads_s": mapped,
                        "M_pairs_per_s_mapped_all_reads": round(args.pairs / mapped / 1e6, 2) if mapped else None, "cli": tail,
                        "bed_md5": subprocess.check_output(["md5sum", out]).split()[0].decode(), "bed_bytes": os.path.getsize(out)}
        best["mapped_all_reads_s_runs"] = times
        best["wall_s_runs"] = walls
        best["md5_runs"] = md5s_run
        res[label] = best

    if args.output_bam and args.sam:
        import zlib
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import bam_model

        def inflated_head(path, want):
            """the first `want` bytes (or a little more) that the BGZF blocks of `path` hold"""
            got = b""
            with open(path, "rb") as f:
                raw = f.read(want)  # (the blocks are never larger than their text here by more than their 26 bytes each)
            while raw and len(got) < want:
                d = zlib.decompressobj(31)
                piece = d.decompress(raw)
                if not d.eof:
                    break
                got += piece
                raw = d.unused_data
            return got
        run("sam", r1, r2)
        with open(out, "rb") as f:
            sam_head = f.read(8 << 20)
        run("sam_output_bgzf", r1, r2, ["--output-bgzf"])
        res["sam_output_bgzf"]["head_inflates_to_sam_head"] = sam_head.startswith(inflated_head(out, 2 << 20)[:1 << 20])
        run("bam", r1, r2, ["--BAM"])
        # whole records of the first MB of the BAM body, printed as SAM, against the SAM file's first lines (SEQ has only ACGT here)
        head = inflated_head(out, 2 << 20)
        l_text, = np.frombuffer(head[4:8], "<u4")
        at = 8 + int(l_text)
        n_ref, = np.frombuffer(head[at:at + 4], "<u4")
        at += 4
        for _ in range(int(n_ref)):
            at += 8 + int(np.frombuffer(head[at:at + 4], "<u4")[0])
        end = at
        while end + 4 <= len(head) and end + 4 + int(np.frombuffer(head[end:end + 4], "<u4")[0]) <= min(len(head), at + (1 << 20)):
            end += 4 + int(np.frombuffer(head[end:end + 4], "<u4")[0])
        text = bam_model.decode(head[:end])
        res["bam"]["records_decoded"] = text.count(b"\n") - int(n_ref)
        res["bam"]["head_decodes_to_sam_head"] = res["bam"]["records_decoded"] > 1000 and sam_head.startswith(text)
        res["output_bam"] = {"sam_bytes": res["sam"]["bed_bytes"], "sam_bgzf_bytes": res["sam_output_bgzf"]["bed_bytes"], "bam_bytes": res["bam"]["bed_bytes"],
                             "wall_s_sam": res["sam"]["wall_s_runs"], "wall_s_sam_output_bgzf": res["sam_output_bgzf"]["wall_s_runs"],
                             "wall_s_bam": res["bam"]["wall_s_runs"]}
        res["config"] = {"preset": args.preset, "sam": True, "pairs": args.pairs, "readlen": args.readlen, "genome": args.genome, "reps": args.reps,
                         "hardware_threads": os.cpu_count(), "cpu_budget": cpu_budget()}
        print(json.dumps(res))
        return
    run("device_ingest", r1, r2)
    if args.output_bgzf and two_routes:
        import gzip
        import hashlib
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import bgzf

        def md5_inflated(path):
            h = hashlib.md5()
            with gzip.open(path, "rb") as f:
                for b in iter(lambda: f.read(1 << 24), b""):
                    h.update(b)
            return h.hexdigest()
        run("device_ingest_output_bgzf", r1, r2, ["--output-bgzf"])
        res["device_ingest_output_bgzf"]["inflates_to_plain_output"] = md5_inflated(out) == res["device_ingest"]["bed_md5"]
        run("device_ingest_then_bgzf_py", r1, r2, after=lambda: bgzf.compress_file(out, out + ".bgz", level=1, threads=16))
        res["device_ingest_then_bgzf_py"]["bgzf_py_bytes"] = os.path.getsize(out + ".bgz")
        os.remove(out + ".bgz")
        if args.baseline_cli:
            run("baseline_cli", r1, r2, cli=args.baseline_cli)
        dev, host = res["device_ingest_output_bgzf"], res["device_ingest_then_bgzf_py"]
        res["output_bgzf"] = {"plain_bytes": res["device_ingest"]["bed_bytes"], "device_bgzf_bytes": dev["bed_bytes"], "bgzf_py_bytes": host["bgzf_py_bytes"],
                              "device_over_bgzf_py_bytes": round(dev["bed_bytes"] / host["bgzf_py_bytes"], 4),
                              "wall_s_plain": res["device_ingest"]["wall_s_runs"], "wall_s_output_bgzf": dev["wall_s_runs"],
                              "wall_s_plain_then_bgzf_py": host["wall_s_runs"]}
        res["config"] = {"preset": args.preset, "sam": args.sam, "pairs": args.pairs, "readlen": args.readlen, "genome": args.genome, "reps": args.reps,
                         "hardware_threads": os.cpu_count(), "cpu_budget": cpu_budget()}
        print(json.dumps(res))
        return
    if args.summary and not two_routes:
        sm = os.path.join(args.dir, "out.summary.csv")
        run("device_ingest_summary", r1, r2, ["--summary", sm])
        res["device_ingest_summary"]["summary_rows"] = sum(1 for _ in open(sm)) - 1
        res["summary_leaves_bed_unchanged"] = res["device_ingest_summary"]["bed_md5"] == res["device_ingest"]["bed_md5"]
    if args.baseline_cli and not two_routes:
        run("baseline_cli", r1, r2, cli=args.baseline_cli)
        res["baseline_same_output"] = res["baseline_cli"]["bed_md5"] == res["device_ingest"]["bed_md5"]
    if two_routes:
        # the two routes of a pairs / SAM run, whole-process wall time: the requirement is slowest(device) < fastest(host) for each input kind
        # (--skip-host-ingest with --baseline-cli: the baseline build stands for the host route, the only one it has)
        host = not (args.skip_host_ingest and args.baseline_cli)
        if host:
            run("host_ingest", r1, r2, ["--host-ingest"])
        if args.baseline_cli:
            run("baseline_cli", r1, r2, cli=args.baseline_cli)
        kinds = [("", "fastq")]
        if args.gz:
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            import bgzf
            for f in (r1, r2):
                bgzf.compress_file(f, f + ".bgz")
            run("device_ingest_bgzf", r1 + ".bgz", r2 + ".bgz")
            if host:
                run("host_ingest_bgzf", r1 + ".bgz", r2 + ".bgz", ["--host-ingest"])
            if args.baseline_cli:
                run("baseline_cli_bgzf", r1 + ".bgz", r2 + ".bgz", cli=args.baseline_cli)
            res["device_ingest_bgzf"]["bgzf_bytes"] = os.path.getsize(r1 + ".bgz") + os.path.getsize(r2 + ".bgz")
            kinds.append(("_bgzf", "bgzf"))
        md5s = set(m for k in res for m in res[k]["md5_runs"])  # every run of every route
        verdict = {}
        for sfx, kind in kinds:
            d, h = res["device_ingest" + sfx]["wall_s_runs"], res["host_ingest" + sfx]["wall_s_runs"] if host else []
            if args.baseline_cli:  # the baseline's fastest run: whichever of the two is faster
                h = h + res["baseline_cli" + sfx]["wall_s_runs"]
            verdict[kind] = {"device_slowest_s": max(d), "host_fastest_s": min(h), "device_beats_host": max(d) < min(h),
                             "speedup_fastest_over_fastest": round(min(h) / min(d), 2)}
        res["same_output"] = len(md5s) == 1
        res["sam_routes" if args.sam else "hic_routes"] = verdict
        res["config"] = {"preset": args.preset, "sam": args.sam, "pairs": args.pairs, "readlen": args.readlen, "genome": args.genome, "reps": args.reps,
                         "fastq_bytes": os.path.getsize(r1) + os.path.getsize(r2), "index_bytes": os.path.getsize(idx),
                         "hardware_threads": os.cpu_count(), "cpu_budget": cpu_budget()}
        print(json.dumps(res))
        return
    if not args.skip_host_ingest:
        run("host_ingest", r1, r2, ["--host-ingest"], reps=1)
    if args.gz:
        for f in (r1, r2):
            subprocess.check_call("gzip -1 -c %s > %s.gz" % (f, f), shell=True)
        run("device_ingest_gz", r1 + ".gz", r2 + ".gz", reps=1)  # one zlib stream per file: inflated on the host, a thread per file
        res["device_ingest_gz"]["gz_bytes"] = os.path.getsize(r1 + ".gz") + os.path.getsize(r2 + ".gz")
        # the same reads block-compressed (BGZF, what bgzip writes): the blocks go to the device compressed and are inflated there
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import bgzf
        for f in (r1, r2):
            bgzf.compress_file(f, f + ".bgz")
        run("device_ingest_bgzf", r1 + ".bgz", r2 + ".bgz")
        res["device_ingest_bgzf"]["bgzf_bytes"] = os.path.getsize(r1 + ".bgz") + os.path.getsize(r2 + ".bgz")
        run("device_ingest_bgzf_256MB_pieces", r1 + ".bgz", r2 + ".bgz", ["--ingest-chunk-mb", "256"])
        res["bgzf_same_output"] = res["device_ingest_bgzf"]["bed_md5"] == res["device_ingest"]["bed_md5"]
        if args.baseline_cli:
            run("baseline_cli_bgzf", r1 + ".bgz", r2 + ".bgz", cli=args.baseline_cli)
            res["baseline_same_output"] = res["baseline_same_output"] and res["baseline_cli_bgzf"]["bed_md5"] == res["device_ingest_bgzf"]["bed_md5"]
    res["same_output"] = res["device_ingest"]["bed_md5"] == res["host_ingest"]["bed_md5"] if "host_ingest" in res else None
    res["config"] = {"pairs": args.pairs, "readlen": args.readlen, "genome": args.genome, "barcodes": args.barcodes, "reps": args.reps,
                     "fastq_bytes": os.path.getsize(r1) + os.path.getsize(r2), "index_bytes": os.path.getsize(idx),
                     "hardware_threads": os.cpu_count(), "cpu_budget": cpu_budget()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
