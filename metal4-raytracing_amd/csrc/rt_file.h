// rt_file.h — the one whole-file reader of the host ingest (USD layers, PNG textures).
#pragma once
#include <sys/stat.h>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

namespace rt {

// The whole file appended to `out`.  With a limit, only a regular file of at most max_bytes (stat) is
// opened: a reference to /dev/zero or a FIFO must not hang the loader.  0: no limit, no such check.
inline bool read_file(const std::string& path, uint64_t max_bytes, std::vector<uint8_t>& out, std::string& err) {
    struct stat sb;
    if (max_bytes && (stat(path.c_str(), &sb) != 0 || !S_ISREG(sb.st_mode) || (uint64_t)sb.st_size > max_bytes)) {
        err = "cannot open " + path + " (not a regular file of at most " + std::to_string(max_bytes >> 30) + " GiB)";
        return false;
    }
    const std::unique_ptr<FILE, int (*)(FILE*)> f(std::fopen(path.c_str(), "rb"), std::fclose);
    if (!f) { err = "cannot open " + path; return false; }
    uint8_t buf[1 << 16];
    size_t k;
    while ((k = std::fread(buf, 1, sizeof buf, f.get())) > 0) out.insert(out.end(), buf, buf + k);
    return true;
}

}  // namespace rt
