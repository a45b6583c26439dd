// bf_write_png_rgba8: what LodePNG::save does for the reference's ColorImageR8G8B8A8 pictures (renderToFile / renderTopDown, DepthSensing.cpp:1187) - an
// 8-bit RGBA PNG without interlace, every scanline with filter 0, one IDAT chunk.  The zlib stream and the chunk CRCs come from zlib, which the
// library links for the depth frames of .sens files.
#include <zlib.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/bf_render.h"
#include "bf_internal.h"

namespace {

void be32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; }

bool chunk(FILE* f, const char type[4], const uint8_t* data, size_t n) {
    uint8_t head[8], tail[4];
    be32(head, (uint32_t)n); memcpy(head + 4, type, 4);
    uLong crc = crc32(0L, head + 4, 4);
    if (n) crc = crc32(crc, data, (uInt)n);
    be32(tail, (uint32_t)crc);
    return fwrite(head, 1, 8, f) == 8 && (n == 0 || fwrite(data, 1, n, f) == n) && fwrite(tail, 1, 4, f) == 4;
}

}  // namespace

extern "C" int bf_write_png_rgba8(const char* path, const uint8_t* rgba, uint32_t width, uint32_t height) {
    BF_REQUIRE(path && rgba && width > 0 && height > 0 && width < 32768 && height < 32768, "bad argument");
    const size_t row = (size_t)width * 4;
    std::vector<uint8_t> raw((row + 1) * height);
    for (uint32_t y = 0; y < height; ++y) {
        raw[(row + 1) * y] = 0;                                       // filter type 0 (None)
        memcpy(&raw[(row + 1) * y + 1], rgba + row * y, row);
    }
    uLongf zn = compressBound((uLong)raw.size());
    std::vector<uint8_t> z(zn);
    if (compress2(z.data(), &zn, raw.data(), (uLong)raw.size(), Z_BEST_SPEED) != Z_OK) { bf::set_error("bf_write_png_rgba8: deflate failed"); return BF_ERR_INVALID_ARG; }
    FILE* f = fopen(path, "wb");
    if (!f) { bf::set_error("cannot write %s", path); return BF_ERR_INVALID_ARG; }
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    uint8_t ihdr[13];
    be32(ihdr, width); be32(ihdr + 4, height);
    ihdr[8] = 8; ihdr[9] = 6; ihdr[10] = 0; ihdr[11] = 0; ihdr[12] = 0;      // 8 bits, colour type 6 (RGBA), deflate, adaptive filtering, no interlace
    const bool ok = fwrite(sig, 1, 8, f) == 8 && chunk(f, "IHDR", ihdr, 13) && chunk(f, "IDAT", z.data(), zn) && chunk(f, "IEND", nullptr, 0);
    if (fclose(f) != 0 || !ok) { bf::set_error("error while writing %s", path); return BF_ERR_INVALID_ARG; }
    return BF_OK;
}
