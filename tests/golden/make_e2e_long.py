"""Generate the long-read end-to-end fixture: four 20-40-kb spliced transcripts of e2e_genome.fa (two per
strand; more than 16 384 distinct 8-mers each, so their stage 2 seeds in the engine's long class) interleaved
with ten reads of e2e_reads.fa, and the reference `gmap` program's SAM on them (nosimd and AVX2 builds).

Run after `make -C oracle ref` (needs oracle/_ref/gmap_{nosimd,avx2}) and make_e2e.py:

    python tests/golden/make_e2e_long.py

The genome file is make_e2e.py's and is not touched, so the long reads' junctions are whatever the segment
holds there (no planted GT...AG); the reads were chosen so that the reference aligns every one of them.

Outputs (data only):
  e2e_long_reads.fa              the 14 reads
  e2e_long_{nosimd,avx2}.sam.gz  `gmap_<build> -g e2e_genome.fa -f samse --no-sam-headers e2e_long_reads.fa`
"""
import gzip
import os
import random
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_e2e import REF, revcomp, write_fasta  # noqa: E402

# (first exon's start, exons, exon length, minus strand)
LONG_READS = ((5000, 8, 3000, False), (60000, 10, 3500, True), (130000, 7, 3000, False), (190000, 9, 4000, True))
ARGS = ["-g", "e2e_genome.fa", "-f", "samse", "--no-sam-headers", "e2e_long_reads.fa"]


def read_fasta(path):
    out, name, seq = [], None, []
    with open(path) as f:
        for line in f:
            if line.startswith(">"):
                if name is not None:
                    out.append((name, "".join(seq)))
                name, seq = line[1:].strip(), []
            else:
                seq.append(line.strip())
    out.append((name, "".join(seq)))
    return out


def long_read(genome, k, start, nexons, exonlen, rc, sub=0.02):
    rng = random.Random(3800 + k)
    parts, pos = [], start
    for e in range(nexons):
        parts.append(genome[pos:pos + exonlen])
        pos += exonlen + rng.randint(500, 3000)
    seq = list("".join(parts))
    for i in range(len(seq)):
        if rng.random() < sub:
            seq[i] = rng.choice([c for c in "ACGT" if c != seq[i]])
    seq = "".join(seq)
    return "long%d_%d_%s" % (k, start + 1, "-" if rc else "+"), revcomp(seq) if rc else seq


def reads():
    genome = read_fasta(os.path.join(HERE, "e2e_genome.fa"))[0][1]
    short = read_fasta(os.path.join(HERE, "e2e_reads.fa"))[:10]
    longs = [long_read(genome, k, *spec) for k, spec in enumerate(LONG_READS)]
    out = []
    for k, r in enumerate(short):  # a long read after the 1st, 4th, 7th and 10th short one
        out.append(r)
        if k % 3 == 0:
            out.append(longs[k // 3])
    return out


def main():
    write_fasta(os.path.join(HERE, "e2e_long_reads.fa"), reads())
    for v in ("nosimd", "avx2"):
        r = subprocess.run([os.path.join(REF, "gmap_" + v)] + ARGS, cwd=HERE, capture_output=True, check=True)
        with gzip.GzipFile(os.path.join(HERE, "e2e_long_%s.sam.gz" % v), "wb", mtime=0) as f:
            f.write(r.stdout)
        print(v, len(r.stdout), "bytes of SAM")


if __name__ == "__main__":
    sys.exit(main())
