"""Writes tests/golden/nthash_counters.json: what the REFERENCE's CntHashEstimator (kmc_core/libs/ntHash/ntHashWrapper.h) counts for fixed generated
sequences — recorded results that pin the numpy oracle of tests/test_stage1_estimate_emulated.py to the reference.

Run by hand on a machine that has the reference's source tree:   python tests/make_nthash_golden.py /path/to/reference
It compiles a short driver of this repository's own (below) against the reference's header into a temporary directory, feeds it the sequences of
golden_sequences(k, s) for k in {21, 27, 31, 33, 62, 66, 256} and s in {1, 7, 11} with r = 16, and records the non-zero (entry, value) pairs of the
2^17-entry counter array (type 0 first). Neither the driver's binary nor anything of the header is kept."""
import json
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DRIVER = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "ntHashWrapper.h"
/* the counters are private: read through a pointer to member handed out by an explicit instantiation (access checks do not apply to its arguments) */
template <class Tag> struct Stowed { static typename Tag::type value; };
template <class Tag> typename Tag::type Stowed<Tag>::value;
template <class Tag, typename Tag::type P> struct Stow { Stow() { Stowed<Tag>::value = P; } static Stow instance; };
template <class Tag, typename Tag::type P> Stow<Tag, P> Stow<Tag, P>::instance;
struct CountersTag { typedef uint32_t *(CntHashEstimator::*type)[2]; };
template struct Stow<CountersTag, &CntHashEstimator::counters>;
int main(int argc, char **argv)
{
	const uint32_t k = atoi(argv[1]), s = atoi(argv[2]), r = atoi(argv[3]);
	CntHashEstimator est(k, s, r);
	char line[1 << 16];
	while (fgets(line, sizeof line, stdin)) {
		std::string codes;
		for (char *p = line; *p && *p != '\n'; ++p)
			codes.push_back(*p == 'A' ? 0 : *p == 'C' ? 1 : *p == 'G' ? 2 : *p == 'T' ? 3 : (char)-1);
		est.Process(codes.data(), (uint32_t)codes.size());
	}
	uint32_t *(&c)[2] = est.*Stowed<CountersTag>::value;
	for (uint32_t t = 0; t < 2; ++t)
		for (uint64_t i = 0; i < (1ull << r); ++i)
			if (c[t][i])
				printf("%llu %u\n", (unsigned long long)((t ? 1ull << r : 0) + i), c[t][i]);
	return 0;
}
"""


def main():
    from test_stage1_estimate_emulated import GOLDEN, golden_sequences

    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    inc = os.path.join(ref, "kmc_core", "libs", "ntHash")
    r, cases = 16, []
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "driver.cpp"), os.path.join(tmp, "driver")
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-w", "-I", inc, src, "-o", exe])
        for k in (21, 27, 31, 33, 62, 66, 256):
            for s in (1, 7, 11):
                seqs = golden_sequences(k, s)
                out = subprocess.run([exe, str(k), str(s), str(r)], input=b"".join(x + b"\n" for x in seqs), stdout=subprocess.PIPE, check=True).stdout
                flat = [int(x) for x in out.split()]
                cases.append(dict(k=k, s=s, n_seqs=len(seqs), n_symbols=sum(len(x) for x in seqs), nonzero=flat))
    with open(GOLDEN, "w") as f:
        json.dump(dict(what="non-zero counters of the reference's CntHashEstimator(k, s, r) over golden_sequences(k, s): entry, value, entry, value ...", r=r,
                       cases=cases), f, separators=(",", ":"))
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")


if __name__ == "__main__":
    main()
