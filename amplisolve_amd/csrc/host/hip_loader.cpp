// amplisolve_amd/csrc/host/hip_loader.cpp
#include "hip_loader.hpp"

#include <dlfcn.h>

#include <cstdlib>
#include <mutex>

#include "host.hpp"

namespace ampli {

static HipApi g_api;
static bool g_ok = false;
static std::string g_why;
static std::once_flag g_once;

static std::string own_dir()
{
    Dl_info info;
    if (dladdr((void *)&own_dir, &info) && info.dli_fname) {
        std::string p(info.dli_fname);
        size_t s = p.rfind('/');
        if (s != std::string::npos) return p.substr(0, s);
    }
    return ".";
}

static void load()
{
    std::vector<std::string> cands;
    if (const char *e = getenv("AMPLISOLVE_HIP_LIB")) cands.emplace_back(e);
    const std::string d = own_dir();
    cands.push_back(d + "/libamplisolve_hip.so");
    cands.push_back(d + "/../lib/libamplisolve_hip.so");
    cands.emplace_back("libamplisolve_hip.so");
    void *h = nullptr;
    for (auto &c : cands) {
        h = dlopen(c.c_str(), RTLD_NOW | RTLD_LOCAL);
        if (h) break;
        g_why = dlerror();
    }
    if (!h) return;
#define BIND_AS(field, name)                                                                 \
    g_api.field = reinterpret_cast<decltype(g_api.field)>(dlsym(h, "ampli_" #name));         \
    if (!g_api.field) { g_why = "missing symbol ampli_" #name; return; }
#define BIND(name) BIND_AS(name, name)
    AMPLI_HIP_API(BIND, BIND_AS)
#undef BIND
#undef BIND_AS
    if (g_api.abi_version() != AMPLI_ABI_VERSION) { g_why = "libamplisolve_hip.so ABI version mismatch"; return; }
    g_ok = true;
}

const HipApi *hip_api(std::string *why)
{
    std::call_once(g_once, load);
    if (!g_ok && why) *why = g_why;
    return g_ok ? &g_api : nullptr;
}

} // namespace ampli
