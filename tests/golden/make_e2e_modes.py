"""Generate the end-to-end fixtures of GMAP's stranded bisulfite / RNA-editing modes
(`gmap --mode=cmet-stranded | atoi-stranded | ttoc-stranded`).

Run in the development container after `make -C oracle ref` (needs oracle/_ref/gmap_{nosimd,avx2}, the
unmodified reference program):

    python tests/golden/make_e2e_modes.py

Inputs: the first 60 reads of e2e_reads.fa (make_e2e.py) with a seeded conversion of the read as given --
cmet: C->T on 90 % of the Cs, atoi: A->G on 30 % of the As, ttoc: T->C on 30 % of the Ts -- and, in ten of
the reads, a stretch of about 100 nt in lower case: convert_to_nucleotides outside STANDARD compares an
observed pair's cdna, the query as given, with the genome's upper-case character (stage2.c:5435), so a
lower-case match is re-pushed with ':'; these reads pin that.

Outputs (data only; gzip, written without a timestamp so that a rerun gives the same bytes -- the tests
unpack them):
  e2e_mode_{cmet,atoi,ttoc}_reads.fa.gz
  e2e_mode_{cmet,atoi,ttoc}_{nosimd,avx2}.sam.gz
        `gmap_<build> --mode=<mode>-stranded -g e2e_genome.fa -f samse --no-sam-headers <reads>`
        (none for ttoc with the AVX2 build: see NO_FIXTURE)
"""
import gzip
import os
import random
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref")

NREADS = 60
SEED = 1905
# mode -> (converted base, what it becomes, fraction converted)
CONVERSION = {"cmet": ("C", "T", 0.90), "atoi": ("A", "G", 0.30), "ttoc": ("T", "C", 0.30)}
LOWER_EVERY, LOWER_LEN = 6, 100   # reads 0, 6, 12, ..., 54 carry the lower-case stretch
# No fixture: the unmodified AVX2 program does not survive ttoc-stranded on these reads (SIGSEGV on the first).
# Its SIMD tally counts with a TTOC arm (count_positions_fwd_simd, oligoindex_hr.c:20182-20226) and stores
# without one (store_positions_fwd_simd's 64-nt step, :21135-21165), so the store pass writes positions the
# count pass never allocated.
NO_FIXTURE = {("ttoc", "avx2")}


def read_fasta(path, n):
    recs, name, seq = [], None, []
    with open(path) as f:
        for line in f:
            line = line.strip()
            if line.startswith(">"):
                if name is not None:
                    recs.append((name, "".join(seq)))
                    if len(recs) == n:
                        return recs
                name, seq = line[1:], []
            elif line:
                seq.append(line)
    if name is not None and len(recs) < n:
        recs.append((name, "".join(seq)))
    return recs


def fasta(records, width=60):
    out = []
    for name, seq in records:
        out.append(">%s\n" % name)
        out.extend(seq[i:i + width] + "\n" for i in range(0, len(seq), width))
    return "".join(out).encode()


def write_gz(name, data):
    with open(os.path.join(HERE, name + ".gz"), "wb") as f:
        with gzip.GzipFile(filename="", mode="wb", fileobj=f, mtime=0) as z:
            z.write(data)


def convert(reads, mode):
    a, b, frac = CONVERSION[mode]
    out = []
    for i, (name, seq) in enumerate(reads):
        rng = random.Random(SEED * 10 ** 6 + 1000 * sorted(CONVERSION).index(mode) + i)
        s = [b if c == a and rng.random() < frac else c for c in seq]
        if i % LOWER_EVERY == 0:
            at = rng.randrange(50, len(s) - LOWER_LEN - 50)
            s[at:at + LOWER_LEN] = [c.lower() for c in s[at:at + LOWER_LEN]]
        out.append((name, "".join(s)))
    return out


def run_gmap(binary, args):
    return subprocess.run([os.path.join(REF, binary)] + args, cwd=HERE, stdout=subprocess.PIPE,
                          stderr=subprocess.DEVNULL, check=True).stdout


def main():
    for b in ("gmap_nosimd", "gmap_avx2"):
        if not os.path.exists(os.path.join(REF, b)):
            sys.exit("oracle/_ref/%s missing: run `make -C oracle ref` first" % b)
    reads = read_fasta(os.path.join(HERE, "e2e_reads.fa"), NREADS)
    assert len(reads) == NREADS
    with tempfile.TemporaryDirectory() as tmp:
        for mode in sorted(CONVERSION):
            data = fasta(convert(reads, mode))
            write_gz("e2e_mode_%s_reads.fa" % mode, data)
            rf = os.path.join(tmp, "e2e_mode_%s_reads.fa" % mode)
            with open(rf, "wb") as f:
                f.write(data)
            for build in ("nosimd", "avx2"):
                if (mode, build) in NO_FIXTURE:
                    continue
                write_gz("e2e_mode_%s_%s.sam" % (mode, build),
                         run_gmap("gmap_" + build, ["--mode=%s-stranded" % mode, "-g", "e2e_genome.fa", "-f", "samse",
                                                    "--no-sam-headers", rf]))
                print("wrote e2e_mode_%s_%s.sam.gz" % (mode, build))


if __name__ == "__main__":
    main()
