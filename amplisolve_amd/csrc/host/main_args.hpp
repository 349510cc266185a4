// amplisolve_amd/csrc/host/main_args.hpp -- what the *_main.cpp files share: reading a key=value token, leaving the process, and the
// whole main() of the project's own commands.
#pragma once
#include <clocale>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

#include "host.hpp"

namespace ampli {

// the value of a key=value token, as the reference reads it: sscanf(argv[i], "key=%s", ...) (EE:300-326); "" when the key differs
inline std::string token(const char *arg, const char *key)
{
    char buf[4096];
    buf[0] = 0;
    std::string fmt = std::string(key) + "=%4000s";
    sscanf(arg, fmt.c_str(), buf);
    return buf;
}

// the end of one of the project's own command lines: exit status 0 on success and 1 on any failure
inline int finish(int rc)
{
    std::cout.flush();
    finish_process(rc ? 1 : 0);
    return rc ? 1 : 0;
}

// One of the project's own command lines: exactly N key=value tokens in the order of `keys`, token i read into its field of Args.
// Any other count prints `usage` and returns 1 before anything else happens.  refbases: the field that AMPLISOLVE_REFBASES_FILE fills
// when it is set (a pre-computed chrom / pos / base table instead of the FASTA), for the commands that read reference bases.
template <class Args> struct KeyArg {
    const char *key;
    std::string Args::*field;
};

template <class Args, size_t N>
int command_main(int argc, char **argv, const char *usage, const KeyArg<Args> (&keys)[N], int (*run)(const Args &),
                 std::string Args::*refbases = nullptr)
{
    setlocale(LC_ALL, "");
    if (argc != (int)N + 1) {
        std::cout << usage << std::endl;
        return 1;
    }
    Args a;
    for (size_t i = 0; i < N; ++i) a.*keys[i].field = token(argv[i + 1], keys[i].key);
    if (refbases)
        if (const char *e = getenv("AMPLISOLVE_REFBASES_FILE")) a.*refbases = e;
    return finish(run(a));
}

} // namespace ampli
