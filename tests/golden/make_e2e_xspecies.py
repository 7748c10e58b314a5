"""Generate the end-to-end fixtures of `gmap --cross-species` (a more sensitive search for canonical
splicing: Stage2_setup's cross_species_p, stage2.c:139-143).

Run in the development container after `make -C oracle ref` (needs oracle/_ref/gmap_{nosimd,avx2}, the
unmodified reference program):

    python tests/golden/make_e2e_xspecies.py

Inputs: the committed reads and genome (make_e2e.py, make_e2e_modes.py); nothing new.

Outputs (data only; gzip, written without a timestamp so that a rerun gives the same bytes -- the tests
unpack them):
  e2e_xspecies_{nosimd,avx2}.sam.gz
        `gmap_<build> --cross-species -g e2e_genome.fa -f samse --no-sam-headers e2e_reads.fa`
  e2e_xspecies_cmet_{nosimd,avx2}.sam.gz
        `gmap_<build> --mode=cmet-stranded --cross-species -g e2e_genome.fa -f samse --no-sam-headers
        e2e_mode_cmet_reads.fa`
"""
import gzip
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref")
TAIL = ["-g", "e2e_genome.fa", "-f", "samse", "--no-sam-headers"]


def write_gz(name, data):
    with open(os.path.join(HERE, name + ".gz"), "wb") as f:
        with gzip.GzipFile(filename="", mode="wb", fileobj=f, mtime=0) as z:
            z.write(data)


def run_gmap(binary, args):
    return subprocess.run([os.path.join(REF, binary)] + args, cwd=HERE, stdout=subprocess.PIPE,
                          stderr=subprocess.DEVNULL, check=True).stdout


def main():
    for b in ("gmap_nosimd", "gmap_avx2"):
        if not os.path.exists(os.path.join(REF, b)):
            sys.exit("oracle/_ref/%s missing: run `make -C oracle ref` first" % b)
    with tempfile.TemporaryDirectory() as tmp:
        cmet = os.path.join(tmp, "e2e_mode_cmet_reads.fa")
        with gzip.open(os.path.join(HERE, "e2e_mode_cmet_reads.fa.gz"), "rb") as z, open(cmet, "wb") as f:
            f.write(z.read())
        for build in ("nosimd", "avx2"):
            write_gz("e2e_xspecies_%s.sam" % build, run_gmap("gmap_" + build, ["--cross-species"] + TAIL + ["e2e_reads.fa"]))
            write_gz("e2e_xspecies_cmet_%s.sam" % build,
                     run_gmap("gmap_" + build, ["--mode=cmet-stranded", "--cross-species"] + TAIL + [cmet]))
            print("wrote e2e_xspecies_%s.sam.gz, e2e_xspecies_cmet_%s.sam.gz" % (build, build))


if __name__ == "__main__":
    main()
