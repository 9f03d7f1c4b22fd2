// crc32c.hip -- rd_crc32c: the checksum of the TFRecord framing (utils/tfevents.py) for records of hundreds of kilobytes (image
// summaries).  Plain host C++: no kernel, no HIP call.
#include <stddef.h>
#include <stdint.h>

// crc32c (Castagnoli, reflected polynomial 0x82F63B78), slicing by 8: host code, no GPU involved.  seed = the crc of the bytes before
// these (0 for none), so that crc(a + b) == rd_crc32c(b, rd_crc32c(a, 0)).
namespace {
struct CrcTables {
    uint32_t t[8][256];
    CrcTables() {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0x82F63B78u : c >> 1;
            t[0][i] = c;
        }
        for (uint32_t i = 0; i < 256; ++i)
            for (int s = 1; s < 8; ++s) t[s][i] = t[0][t[s - 1][i] & 0xff] ^ (t[s - 1][i] >> 8);
    }
};
}  // namespace

extern "C" uint32_t rd_crc32c(const void* data, size_t n, uint32_t seed) {
    static const CrcTables T;
    const unsigned char* p = (const unsigned char*)data;
    uint32_t c = ~seed;
    while (n >= 8) {
        // bytes are combined one by one: no unaligned word loads, no dependence on the host's byte order
        const uint32_t lo = c ^ ((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24);
        c = T.t[7][lo & 0xff] ^ T.t[6][(lo >> 8) & 0xff] ^ T.t[5][(lo >> 16) & 0xff] ^ T.t[4][lo >> 24] ^
            T.t[3][p[4]] ^ T.t[2][p[5]] ^ T.t[1][p[6]] ^ T.t[0][p[7]];
        p += 8;
        n -= 8;
    }
    while (n--) c = T.t[0][(c ^ *p++) & 0xff] ^ (c >> 8);
    return ~c;
}
