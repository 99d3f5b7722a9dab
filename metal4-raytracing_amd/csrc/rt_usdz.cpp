// rt_usdz.cpp — the .usdz package reader: a zip of stored or deflated entries (see rt_usd.h).
#include "rt_usd_internal.h"

#include <zlib.h>

#include <cstring>

namespace rt {
namespace usd {

bool read_zip(const uint8_t* data, size_t n, std::vector<PackageFile>& files, std::string& err) {
    if (n < 22) { err = "zip: too short"; return false; }
    size_t eocd = (size_t)-1;
    for (size_t i = n - 22 + 1; i-- > 0 && n - i <= 22 + 65535;)
        if (rd32(data + i) == 0x06054b50u) { eocd = i; break; }
    if (eocd == (size_t)-1) { err = "zip: no end-of-central-directory record"; return false; }
    const uint32_t entries = rd16(data + eocd + 10), cd_off = rd32(data + eocd + 16);
    size_t p = cd_off;
    for (uint32_t e = 0; e < entries; ++e) {
        if (p + 46 > n || rd32(data + p) != 0x02014b50u) { err = "zip: bad central directory"; return false; }
        const uint32_t method = rd16(data + p + 10), csize = rd32(data + p + 20), usize = rd32(data + p + 24);
        const uint32_t nlen = rd16(data + p + 28), elen = rd16(data + p + 30), clen = rd16(data + p + 32);
        const uint32_t lho = rd32(data + p + 42);
        if (p + 46 + nlen > n) { err = "zip: bad entry name"; return false; }
        PackageFile f;
        f.name.assign((const char*)data + p + 46, nlen);
        p += 46 + nlen + elen + clen;
        if (csize == 0xffffffffu || usize == 0xffffffffu || lho == 0xffffffffu) { err = "zip: zip64 entries unsupported"; return false; }
        if (!f.name.empty() && f.name.back() == '/') continue;
        if ((size_t)lho + 30 > n || rd32(data + lho) != 0x04034b50u) { err = "zip: bad local header"; return false; }
        const size_t off = (size_t)lho + 30 + rd16(data + lho + 26) + rd16(data + lho + 28);
        if (off + csize > n) { err = "zip: truncated entry " + f.name; return false; }
        if (method == 0) {
            f.data.assign(data + off, data + off + csize);
        } else if (method == 8) {
            if ((uint64_t)usize > 1032ull * csize + 1024) { err = "zip: implausible size of " + f.name; return false; }
            f.data.resize(usize);
            z_stream zs;
            std::memset(&zs, 0, sizeof zs);
            if (inflateInit2(&zs, -MAX_WBITS) != Z_OK) { err = "zip: inflateInit2"; return false; }
            zs.next_in = const_cast<Bytef*>(data + off);
            zs.avail_in = csize;
            zs.next_out = f.data.data();
            zs.avail_out = usize;
            const int r = inflate(&zs, Z_FINISH);
            inflateEnd(&zs);
            if (r != Z_STREAM_END || zs.total_out != usize) { err = "zip: inflate failed for " + f.name; return false; }
        } else {
            err = "zip: compression method " + std::to_string(method) + " unsupported (" + f.name + ")";
            return false;
        }
        files.push_back(std::move(f));
    }
    return true;
}

}  // namespace usd
}  // namespace rt
