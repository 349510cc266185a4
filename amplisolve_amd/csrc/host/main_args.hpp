// amplisolve_amd/csrc/host/main_args.hpp -- what the *_main.cpp files share: reading a key=value token and leaving the process.
#pragma once
#include <cstdio>
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

} // namespace ampli
