"""BGZF input through moni-hip-align end to end.  Run after profiles/frontend.py, which leaves its reads in /tmp/frontend_reads.fq and the
index in the bench's cache: the same CLI call on the plain file and on a bgzipped copy (zlib level 6, 65280-byte members, made here by sixteen processes),
twice each in turn, MONI_CLI_VERBOSE=1; steady-state reads/s of each run (the ranges from 3/8 of the run to the last but one, as DESIGN 5 counts them: 9-22
of 24), the two outputs compared.  Writes bench_out/frontend_bgzf_input.json.

    python3 profiles/frontend.py 24000000 && python3 profiles/frontend_bgzf.py"""
import multiprocessing, os, re, subprocess, sys, time, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from profiles.inflate_rate import member, BS

fq, fz = "/tmp/frontend_reads.fq", "/tmp/frontend_reads.fq.gz"
mfi = "/tmp/moni_bench_cache/idx_61420004_12_lifted_0"
exe = os.path.join(ROOT, "moni_align_amd", "host", "moni-hip-align")


def blocks(f):
    while True:
        b = f.read(BS)
        if not b:
            return
        yield b


t0 = time.time()
with open(fq, "rb") as f, open(fz, "wb") as g, multiprocessing.Pool(16) as pool:
    for m in pool.imap(member, blocks(f), chunksize=256):
        g.write(m)
    g.write(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
print("bgzipped in %.0fs: %.2f GB -> %.2f GB" % (time.time() - t0, os.path.getsize(fq) / 1e9, os.path.getsize(fz) / 1e9), flush=True)


def run(inp, out, extra=()):
    cmd = [exe, mfi, "-p", inp, "-o", out, "-t", "16", "-S", "1000", "-F", "0.5"] + list(extra)
    t = time.time()
    r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, MONI_CLI_VERBOSE="1"), timeout=300)
    wall = time.time() - t
    if r.returncode:
        print(r.stderr[-3000:]); sys.exit("CLI failed with %d" % r.returncode)
    rng = sorted((int(m.group(1)), int(m.group(2)), float(m.group(3))) for m in re.finditer(r"range (\d+) \(worker \d+, (\d+) reads\).*done at ([0-9.]+) s", r.stderr))
    n = len(rng)
    k0, k1 = (3 * n + 7) // 8, n - 2
    reads = sum(x[1] for x in rng[k0:k1 + 1])
    dt = rng[k1][2] - rng[k0 - 1][2]
    tail = [l for l in r.stderr.splitlines() if "Reads per second" in l or "Stage seconds" in l or "BGZF input" in l or "Elapsed" in l]
    res = {"input": inp, "extra": list(extra), "wall_s": wall, "ranges": n, "steady_ranges": [k0, k1], "steady_reads": reads, "steady_s": dt, "steady_Mreads_per_s": reads / dt / 1e6,
           "done_at_s": [x[2] for x in rng], "lines": tail}
    print(json.dumps(res), flush=True)
    return res


res = {"plain": run(fq, "/tmp/fe_plain.sam"), "bgzf": run(fz, "/tmp/fe_bgzf.sam"), "plain_again": run(fq, "/tmp/fe_plain2.sam"), "bgzf_again": run(fz, "/tmp/fe_bgzf2.sam")}
res["outputs_identical"] = subprocess.run(["cmp", "/tmp/fe_plain.sam", "/tmp/fe_bgzf.sam"]).returncode == 0
res["ratio"] = res["bgzf"]["steady_Mreads_per_s"] / res["plain"]["steady_Mreads_per_s"]
res["ratio_again"] = res["bgzf_again"]["steady_Mreads_per_s"] / res["plain_again"]["steady_Mreads_per_s"]
os.makedirs(os.path.join(ROOT, "bench_out"), exist_ok=True)
json.dump(res, open(os.path.join(ROOT, "bench_out", "frontend_bgzf_input.json"), "w"))
print("outputs identical:", res["outputs_identical"], "ratio", res["ratio"], res["ratio_again"])
