// gz_format.h -- the facts the gzip codec's host and device code share, each
// written once: the inflate status bits, the member index record, and the TLZ
// member format (constants and the byte offsets of every header field).
// Plain C++17, <cstdint> only: the functions are constexpr, so the device
// code may call them too.
#pragma once
#include <cstdint>

namespace gz {

// status word of the inflate kernels: OR of these over the members
constexpr int kInfCorrupt = 1, kInfSize = 2, kInfCrc = 4, kInfRange = 8;

// ---- the member index (ofl_gzip_member_index): kIdxWords int64 per member --
constexpr int kIdxWords = 4;
constexpr int kIdxIn = 0;     // offset of the deflate data in the stream
constexpr int kIdxLen = 1;    // length of the deflate data | kIdxTlz if the member is TLZ
constexpr int kIdxOut = 2;    // offset of the member's output
constexpr int kIdxSize = 3;   // ISIZE | CRC-32 << 32
constexpr int64_t kIdxTlz = (int64_t)1 << 62;
constexpr void idx_pack(int64_t* r, uint64_t in, uint64_t in_len, bool tlz, uint64_t out, uint32_t isize, uint32_t crc) {
    r[kIdxIn] = (int64_t)in;
    r[kIdxLen] = (int64_t)in_len | (tlz ? kIdxTlz : 0);
    r[kIdxOut] = (int64_t)out;
    r[kIdxSize] = (int64_t)((uint64_t)isize | ((uint64_t)crc << 32));
}
// the fields of the two packed words.  Macros, not functions: the kernels
// read a record in their first lines, and with a call there, even an
// always-inlined one, the compiler gave k_tlz_ops other code throughout
// (another branch structure of its range check, another register allocation)
#define GZ_IDX_IN_LEN(len_word) ((uint32_t)(len_word))  // a member is < 4 GiB: the low word
#define GZ_IDX_IS_TLZ(len_word) (((len_word) & gz::kIdxTlz) != 0)
#define GZ_IDX_ISIZE(size_word) ((uint32_t)((uint64_t)(size_word) & 0xffffffffu))
#define GZ_IDX_CRC(size_word) ((uint32_t)((uint64_t)(size_word) >> 32))

// little-endian fields
constexpr uint32_t rd16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
constexpr uint32_t rd32(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// ---- a gzip member with an extra field (RFC 1952) --------------------------
//   1f 8b 08 04 | mtime | xfl | os | XLEN (u16) | subfields | deflate data |
//   CRC-32 | ISIZE;   a subfield: SI1 SI2 | LEN (u16) | LEN bytes
constexpr int kGzXlen = 10;                 // offset of XLEN
constexpr int kGzFixed = 12;                // bytes before the extra field
constexpr int kGzTrailer = 8;               // CRC-32, ISIZE
constexpr int kSubLen = 2, kSubFixed = 4;   // a subfield's LEN, its bytes before the payload
// the 'BC' subfield (BGZF): member bytes - 1, u16
constexpr int kBcLen = 2, kBcSize = 4;

namespace tlz {
constexpr int kSegLog = 11, kSeg = 1 << kSegLog;   // values per segment
constexpr int kMemSeg = 64;
constexpr int kMemTok = kSeg * kMemSeg;            // values per member
constexpr int kSlotPerTok = 6;                     // worst-case member bytes per value (4 literals x 11 bits)
constexpr int kSlotPad = 8192;                     // + headers
constexpr int kBatch = 512;                        // members per launch

// the 'OZ' subfield of a TLZ member, offsets from its SI1; it is the only
// subfield, so the segment table ends where the deflate data starts
constexpr int kVersion = 1;
constexpr int kOzVersion = 4;    // u8: kVersion
constexpr int kOzSegLog = 5;     // u8: kSegLog
constexpr int kOzNseg = 6;       // u16: segments
constexpr int kOzBytes = 8;      // u32: member bytes
constexpr int kOzValues = 12;    // u32: float32 values (ISIZE / 4)
constexpr int kOzTable = 16;     // nseg x u32: bit offset of every segment's first symbol in the deflate data
constexpr int kOzFixed = kOzTable - kSubFixed;     // payload bytes before the table
constexpr int kHdrFixed = kGzFixed + kOzTable;     // member header bytes before the segment table
static_assert(kHdrFixed == 28, "the TLZ header is 28 bytes and the segment table");
constexpr int table_bytes(int nseg) { return 4 * nseg; }
constexpr int hdr_bytes(int nseg) { return kHdrFixed + table_bytes(nseg); }
}  // namespace tlz

}  // namespace gz
