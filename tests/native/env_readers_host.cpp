// Host driver of the environment readers (fastfourierconvolution_amd/csrc/ffc_env.h) for
// tests/test_env_readers_cpu.py: the library's own header, no HIP.
//
// argv: a sequence of queries, each answered by one line on stdout
//   int NAME DFLT   -> ffc::env_int(NAME, DFLT)
//   first NAME      -> ffc::env_first(NAME) as a number (0: unset or empty)
//   is NAME WORD    -> ffc::env_is(NAME, WORD) as 0 / 1
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ffc_env.h"

int main(int argc, char** argv) {
    int i = 1;
    while (i < argc) {
        const char* op = argv[i];
        if (!std::strcmp(op, "int") && i + 2 < argc) {
            std::printf("%d\n", ffc::env_int(argv[i + 1], std::atoi(argv[i + 2])));
            i += 3;
        } else if (!std::strcmp(op, "first") && i + 1 < argc) {
            std::printf("%d\n", (int)ffc::env_first(argv[i + 1]));
            i += 2;
        } else if (!std::strcmp(op, "is") && i + 2 < argc) {
            std::printf("%d\n", ffc::env_is(argv[i + 1], argv[i + 2]) ? 1 : 0);
            i += 3;
        } else {
            std::fprintf(stderr, "bad query at argument %d: %s\n", i, op);
            return 2;
        }
    }
    return 0;
}
