// amplisolve_amd/csrc/host/bam_walk.hpp -- the walk over one BAM file that computeCounts (bam.cpp) and computeIndelCounts (run_ci.cpp)
// share: the panel's positions as device keys, the BGZF blocks inflated in batches into two pinned buffers (batch k + 1 is inflated
// while batch k is uploaded and counted), the header that may span batches, the incomplete record carried from batch to batch, the
// record scanner.  What differs between the commands is what they launch per batch: a BamSink.  The body is in bam.cpp.
#pragma once
#include <unistd.h>

#include <algorithm>
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

#include "hip_loader.hpp"
#include "host.hpp"

namespace ampli {

struct VcfLine { // one listed position of vcf=
    std::string chrom, id, ref, alt;
    int64_t pos = 0;
    int64_t key_index = -1; // index into the sorted unique keys, -1: the chromosome is not in the BAM header
};

// the context of a walk and what was allocated under it; outlives the walk, so that the command can copy its outputs back
struct BamDevice {
    const HipApi *api = nullptr;
    ampli_ctx *ctx = nullptr;
    std::vector<void *> allocs;
    BamDevice() = default;
    BamDevice(const BamDevice &) = delete;
    BamDevice &operator=(const BamDevice &) = delete;
    ~BamDevice()
    {
        if (ctx) {
            for (void *p : allocs) api->dev_free(ctx, p);
            api->ctx_destroy(ctx);
        }
    }
    void check(int rc, const char *what)
    {
        if (rc != AMPLI_OK) throw Error{rc, std::string(what) + ": " + api->strerror_(rc) + (ctx ? std::string(" -- ") + api->last_error(ctx) : "")};
    }
    void *alloc(size_t n)
    {
        void *p = nullptr;
        check(api->dev_alloc(ctx, n ? n : 16, &p), "ampli_dev_alloc");
        allocs.push_back(p);
        return p;
    }
    void release(void *p) // a slot's buffer is replaced by a larger one
    {
        if (!p) return;
        allocs.erase(std::remove(allocs.begin(), allocs.end(), p), allocs.end());
        check(api->dev_free(ctx, p), "ampli_dev_free");
    }
};

// what to launch per batch
struct BamSink {
    // optional; once, when the BAM header is read, before `panel` and whatever P is: the names of the file's reference sequences, in
    // the order of their ids (what a sink needs to turn chromosome names of its own into keys)
    std::function<void(const std::vector<std::string> &ref_names)> header;
    // once, when the BAM header is read and the panel has P > 0 positions in it: allocate and clear the outputs
    std::function<void(BamDevice &dev, int64_t P)> panel;
    // per batch with records (only when P > 0): n_reads records of d_bam at d_off, enqueued on the context's stream
    std::function<void(BamDevice &dev, const uint8_t *d_bam, const uint64_t *d_off, int64_t n_reads, const uint64_t *d_keys, int64_t P)> batch;
};

struct BamWalk {
    std::vector<VcfLine> lines; // the listed positions in the list's order, key_index filled in
    std::vector<std::string> ref_names;
    int64_t P = 0, n_records = 0, malformed = 0;
    double t_start = 0, t_inflate = 0, t_wait = 0;
    int threads = 0;
    size_t total_bytes = 0; // uncompressed
    double seconds() const; // since t_start
};

// the output files of a command that writes several: all of them or none
struct TempFiles { // <path>.tmp<pid> for every output; renamed into place by commit(), removed by the destructor otherwise
    std::vector<std::pair<std::string, std::string>> files; // temporary name, final name
    bool done = false;
    FILE *open(const std::string &path)
    {
        const std::string tmp = path + ".tmp" + std::to_string((long long)getpid());
        FILE *o = fopen(tmp.c_str(), "w");
        if (!o) throw Error{AMPLI_E_INVALID, "cannot write " + path};
        files.emplace_back(tmp, path);
        return o;
    }
    void close(FILE *o, const std::string &path)
    {
        if (fclose(o) != 0) throw Error{AMPLI_E_INVALID, "cannot write " + path};
    }
    void commit()
    {
        for (size_t i = 0; i < files.size(); ++i)
            if (rename(files[i].first.c_str(), files[i].second.c_str()) != 0) {
                for (size_t k = 0; k < i; ++k) unlink(files[k].second.c_str());
                throw Error{AMPLI_E_INVALID, "cannot write " + files[i].second};
            }
        done = true;
    }
    ~TempFiles()
    {
        if (!done)
            for (auto &f : files) unlink(f.first.c_str());
    }
};

// Loads the HIP library, reads the positions, opens the file, creates dev's context and walks the file.  Throws Error.
BamWalk walk_bam(const std::string &vcf, const std::string &bam, int threads, BamDevice &dev, const BamSink &sink);

} // namespace ampli
