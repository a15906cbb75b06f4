// The host twin of the predecessors executor's sessions (fx_pred_advance_host)
// on buffers allocated at exactly the sizes the header states (planes of
// fx_plane_words words, [S] arrays, a state of fx_pred_session_bytes bytes).
// Built with -fsanitize=address,undefined (`make pred-advance-check`), so a
// store one word outside a buffer, or a read of one, stops the program.
// The streams and what they must leave are written out below: the hand-built
// streams that carry registrations, window bits and repeats across a cut, and
// one fitting and one exceeding stream per reachable limit of the generic
// SMALL layout (64 vertices, 128 index slots, 1024-seq windows, 256 list
// entries; its frame stack cannot run out before the vertices do).  Each runs
// whole, cut one row before its failing (or last) row, one row per call, and
// untouched by two calls and then whole; after every call the outputs also
// equal a fresh one-call session's with the same lengths.  Then the contract
// edges.  Host only: no device.
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "fantoch_amd.h"

namespace {

int failures = 0;
constexpr uint32_t A5 = 0xA5A5A5A5u;

#define EXPECT(cond, ...)                 \
  do {                                    \
    if (!(cond)) {                        \
      ++failures;                         \
      printf("FAILED %s: ", #cond);       \
      printf(__VA_ARGS__);                \
      printf("\n");                       \
    }                                     \
  } while (0)

struct Row {
  uint32_t dot;    // FX_DOT(source, seq)
  uint64_t clock;  // (seq << 8) | process id
  std::vector<uint32_t> deps;
};
// cut: the row that fails, or the last row; err, nexec, order (arrival rows in
// execution order) and release (by arrival row; -1: never executed) after the
// whole stream at FX_PRED_TIER_SMALL
struct Stream {
  const char* name;
  uint32_t n, dmax, cut, err, nexec;
  std::vector<Row> rows;
  std::vector<uint32_t> order;
  std::vector<int> release;
};

const std::vector<Stream> STREAMS = {
  {"base", 3, 3, 3, 0, 4,
   {{0x01000001, 0x101, {0x02000001}}, {0x01000002, 0x201, {0x01000001}}, {0x03000001, 0x303, {0x01000002}}, {0x02000001, 0x402, {}}},
   {0, 1, 2, 3},
   {3, 3, 3, 3}},
  {"low-clock closer", 3, 3, 3, 0, 4,
   {{0x01000001, 0x201, {0x02000001}}, {0x01000002, 0x301, {0x01000001}}, {0x03000001, 0x403, {0x01000002}}, {0x02000001, 0x102, {}}},
   {3, 0, 1, 2},
   {3, 3, 3, 3}},
  {"bits above the frontier", 3, 3, 6, 0, 7,
   {{0x01000003, 0x301, {}}, {0x01000005, 0x501, {}}, {0x01000002, 0x201, {}}, {0x02000001, 0x902, {0x01000001, 0x01000004, 0x01000005}}, {0x01000001, 0x101, {}}, {0x03000001, 0xA03, {0x01000002, 0x01000003, 0x01000005}}, {0x01000004, 0x401, {0x02000001}}},
   {0, 1, 2, 4, 5, 6, 3},
   {0, 1, 2, 6, 4, 5, 6}},
  {"repeat of a pending dot", 3, 3, 3, 3, 0,
   {{0x01000001, 0x101, {0x02000001}}, {0x01000002, 0x201, {0x01000001}}, {0x03000001, 0x303, {0x01000002}}, {0x01000002, 0x901, {}}, {0x02000001, 0x402, {}}},
   {},
   {-1, -1, -1, -1, -1}},
  {"repeat of an executed dot", 3, 3, 2, 3, 1,
   {{0x01000001, 0x101, {}}, {0x02000001, 0x202, {0x0200FFFF}}, {0x01000001, 0x301, {}}, {0x03000001, 0x403, {}}},
   {0},
   {0, -1, -1, -1}},
  {"source 0", 3, 3, 2, 5, 0,
   {{0x01000001, 0x101, {0x02000001}}, {0x01000002, 0x201, {0x01000001}}, {0x00000001, 0x701, {}}, {0x03000001, 0x303, {0x01000002}}, {0x02000001, 0x402, {}}},
   {},
   {-1, -1, -1, -1, -1}},
  {"vertices fit", 2, 1, 63, 0, 64,
   {{0x01000001, 0x201, {0x02000028}}, {0x01000002, 0x301, {0x02000028}}, {0x01000003, 0x401, {0x02000028}}, {0x01000004, 0x501, {0x02000028}}, {0x01000005, 0x601, {0x02000028}}, {0x01000006, 0x701, {0x02000028}}, {0x01000007, 0x801, {0x02000028}}, {0x01000008, 0x901, {0x02000028}}, {0x01000009, 0xA01, {0x02000028}}, {0x0100000A, 0xB01, {0x02000028}}, {0x0100000B, 0xC01, {0x02000028}}, {0x0100000C, 0xD01, {0x02000028}}, {0x0100000D, 0xE01, {0x02000028}}, {0x0100000E, 0xF01, {0x02000028}}, {0x0100000F, 0x1001, {0x02000028}}, {0x01000010, 0x1101, {0x02000028}}, {0x01000011, 0x1201, {0x02000028}}, {0x01000012, 0x1301, {0x02000028}}, {0x01000013, 0x1401, {0x02000028}}, {0x01000014, 0x1501, {0x02000028}}, {0x01000015, 0x1601, {0x02000028}}, {0x01000016, 0x1701, {0x02000028}}, {0x01000017, 0x1801, {0x02000028}}, {0x01000018, 0x1901, {0x02000028}}, {0x01000019, 0x1A01, {0x02000028}}, {0x0100001A, 0x1B01, {0x02000028}}, {0x0100001B, 0x1C01, {0x02000028}}, {0x0100001C, 0x1D01, {0x02000028}}, {0x0100001D, 0x1E01, {0x02000028}}, {0x0100001E, 0x1F01, {0x02000028}}, {0x0100001F, 0x2001, {0x02000028}}, {0x01000020, 0x2101, {0x02000028}}, {0x01000021, 0x2201, {0x02000028}}, {0x01000022, 0x2301, {0x02000028}}, {0x01000023, 0x2401, {0x02000028}}, {0x01000024, 0x2501, {0x02000028}}, {0x01000025, 0x2601, {0x02000028}}, {0x01000026, 0x2701, {0x02000028}}, {0x01000027, 0x2801, {0x02000028}}, {0x01000028, 0x2901, {0x02000028}}, {0x01000029, 0x2A01, {0x02000028}}, {0x0100002A, 0x2B01, {0x02000028}}, {0x0100002B, 0x2C01, {0x02000028}}, {0x0100002C, 0x2D01, {0x02000028}}, {0x0100002D, 0x2E01, {0x02000028}}, {0x0100002E, 0x2F01, {0x02000028}}, {0x0100002F, 0x3001, {0x02000028}}, {0x01000030, 0x3101, {0x02000028}}, {0x01000031, 0x3201, {0x02000028}}, {0x01000032, 0x3301, {0x02000028}}, {0x01000033, 0x3401, {0x02000028}}, {0x01000034, 0x3501, {0x02000028}}, {0x01000035, 0x3601, {0x02000028}}, {0x01000036, 0x3701, {0x02000028}}, {0x01000037, 0x3801, {0x02000028}}, {0x01000038, 0x3901, {0x02000028}}, {0x01000039, 0x3A01, {0x02000028}}, {0x0100003A, 0x3B01, {0x02000028}}, {0x0100003B, 0x3C01, {0x02000028}}, {0x0100003C, 0x3D01, {0x02000028}}, {0x0100003D, 0x3E01, {0x02000028}}, {0x0100003E, 0x3F01, {0x02000028}}, {0x0100003F, 0x4001, {0x02000028}}, {0x02000028, 0x102, {}}},
   {63, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 61, 62},
   {63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63}},
  {"vertices exceed", 2, 1, 64, 2, 0,
   {{0x01000001, 0x201, {0x02000028}}, {0x01000002, 0x301, {0x02000028}}, {0x01000003, 0x401, {0x02000028}}, {0x01000004, 0x501, {0x02000028}}, {0x01000005, 0x601, {0x02000028}}, {0x01000006, 0x701, {0x02000028}}, {0x01000007, 0x801, {0x02000028}}, {0x01000008, 0x901, {0x02000028}}, {0x01000009, 0xA01, {0x02000028}}, {0x0100000A, 0xB01, {0x02000028}}, {0x0100000B, 0xC01, {0x02000028}}, {0x0100000C, 0xD01, {0x02000028}}, {0x0100000D, 0xE01, {0x02000028}}, {0x0100000E, 0xF01, {0x02000028}}, {0x0100000F, 0x1001, {0x02000028}}, {0x01000010, 0x1101, {0x02000028}}, {0x01000011, 0x1201, {0x02000028}}, {0x01000012, 0x1301, {0x02000028}}, {0x01000013, 0x1401, {0x02000028}}, {0x01000014, 0x1501, {0x02000028}}, {0x01000015, 0x1601, {0x02000028}}, {0x01000016, 0x1701, {0x02000028}}, {0x01000017, 0x1801, {0x02000028}}, {0x01000018, 0x1901, {0x02000028}}, {0x01000019, 0x1A01, {0x02000028}}, {0x0100001A, 0x1B01, {0x02000028}}, {0x0100001B, 0x1C01, {0x02000028}}, {0x0100001C, 0x1D01, {0x02000028}}, {0x0100001D, 0x1E01, {0x02000028}}, {0x0100001E, 0x1F01, {0x02000028}}, {0x0100001F, 0x2001, {0x02000028}}, {0x01000020, 0x2101, {0x02000028}}, {0x01000021, 0x2201, {0x02000028}}, {0x01000022, 0x2301, {0x02000028}}, {0x01000023, 0x2401, {0x02000028}}, {0x01000024, 0x2501, {0x02000028}}, {0x01000025, 0x2601, {0x02000028}}, {0x01000026, 0x2701, {0x02000028}}, {0x01000027, 0x2801, {0x02000028}}, {0x01000028, 0x2901, {0x02000028}}, {0x01000029, 0x2A01, {0x02000028}}, {0x0100002A, 0x2B01, {0x02000028}}, {0x0100002B, 0x2C01, {0x02000028}}, {0x0100002C, 0x2D01, {0x02000028}}, {0x0100002D, 0x2E01, {0x02000028}}, {0x0100002E, 0x2F01, {0x02000028}}, {0x0100002F, 0x3001, {0x02000028}}, {0x01000030, 0x3101, {0x02000028}}, {0x01000031, 0x3201, {0x02000028}}, {0x01000032, 0x3301, {0x02000028}}, {0x01000033, 0x3401, {0x02000028}}, {0x01000034, 0x3501, {0x02000028}}, {0x01000035, 0x3601, {0x02000028}}, {0x01000036, 0x3701, {0x02000028}}, {0x01000037, 0x3801, {0x02000028}}, {0x01000038, 0x3901, {0x02000028}}, {0x01000039, 0x3A01, {0x02000028}}, {0x0100003A, 0x3B01, {0x02000028}}, {0x0100003B, 0x3C01, {0x02000028}}, {0x0100003C, 0x3D01, {0x02000028}}, {0x0100003D, 0x3E01, {0x02000028}}, {0x0100003E, 0x3F01, {0x02000028}}, {0x0100003F, 0x4001, {0x02000028}}, {0x01000040, 0x4101, {0x02000028}}, {0x02000028, 0x102, {}}},
   {},
   {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}},
  {"index fit", 2, 1, 1, 0, 1,
   {{0x01000001, 0x101, {0x02000009}}, {0x01000080, 0x201, {}}},
   {1},
   {-1, 1}},
  {"index exceed", 2, 1, 1, 2, 0,
   {{0x01000001, 0x101, {0x02000009}}, {0x01000081, 0x201, {}}},
   {},
   {-1, -1}},
  {"index freed", 2, 1, 1, 0, 1,
   {{0x01000001, 0x101, {}}, {0x01000081, 0x201, {0x02000009}}},
   {0},
   {0, -1}},
  {"index per source", 2, 1, 2, 2, 1,
   {{0x01000001, 0x101, {0x02000009}}, {0x02000081, 0x201, {}}, {0x01000101, 0x301, {}}},
   {1},
   {-1, 1, -1}},
  {"window fit", 2, 1, 1, 0, 2,
   {{0x02000001, 0x101, {}}, {0x01000400, 0x201, {}}},
   {0, 1},
   {0, 1}},
  {"window exceed", 2, 1, 1, 2, 1,
   {{0x02000001, 0x101, {}}, {0x01000401, 0x201, {}}},
   {0},
   {0, -1}},
  {"lists fit", 2, 17, 31, 0, 16,
   {{0x02000001, 0x102, {0x0200FFFF}}, {0x02000002, 0x3E801, {0x01000001, 0x01000002, 0x01000003, 0x01000004, 0x01000005, 0x01000006, 0x01000007, 0x01000008, 0x01000009, 0x0100000A, 0x0100000B, 0x0100000C, 0x0100000D, 0x0100000E, 0x0100000F, 0x01000010, 0x02000001}}, {0x02000003, 0x3E901, {0x01000001, 0x01000002, 0x01000003, 0x01000004, 0x01000005, 0x01000006, 0x01000007, 0x01000008, 0x01000009, 0x0100000A, 0x0100000B, 0x0100000C, 0x0100000D, 0x0100000E, 0x0100000F, 0x01000010, 0x02000001}}, {0x02000004, 0x3EA01, {0x01000001, 0x01000002, 0x01000003, 0x01000004, 0x01000005, 0x01000006, 0x01000007, 0x01000008, 0x01000009, 0x0100000A, 0x0100000B, 0x0100000C, 0x0100000D, 0x0100000E, 0x0100000F, 0x01000010, 0x02000001}}, {0x02000005, 0x3EB01, {0x01000001, 0x01000002, 0x01000003, 0x01000004, 0x01000005, 0x01000006, 0x01000007, 0x01000008, 0x01000009, 0x0100000A, 0x0100000B, 0x0100000C, 0x0100000D, 0x0100000E, 0x0100000F, 0x01000010, 0x02000001}}, {0x02000006, 0x3EC01, {0x01000001, 0x01000002, 0x01000003, 0x01000004, 0x01000005, 0x01000006, 0x01000007, 0x01000008, 0x01000009, 0x0100000A, 0x0100000B, 0x0100000C, 0x0100000D, 0x0100000E, 0x0100000F, 0x01000010, 0x02000001}}, {0x02000007, 0x3ED01, {0x01000001, 0x01000002, 0x01000003, 0x01000004, 0x01000005, 0x01000006, 0x01000007, 0x01000008, 0x01000009, 0x0100000A, 0x0100000B, 0x0100000C, 0x0100000D, 0x0100000E, 0x0100000F, 0x01000010, 0x02000001}}, {0x02000008, 0x3EE01, {0x01000001, 0x01000002, 0x01000003, 0x01000004, 0x01000005, 0x01000006, 0x01000007, 0x01000008, 0x01000009, 0x0100000A, 0x0100000B, 0x0100000C, 0x0100000D, 0x0100000E, 0x0100000F, 0x01000010, 0x02000001}}, {0x02000009, 0x3EF01, {0x01000001, 0x01000002, 0x01000003, 0x01000004, 0x01000005, 0x01000006, 0x01000007, 0x01000008, 0x01000009, 0x0100000A, 0x0100000B, 0x0100000C, 0x0100000D, 0x0100000E, 0x0100000F, 0x01000010, 0x02000001}}, {0x0200000A, 0x3F001, {0x01000001, 0x01000002, 0x01000003, 0x01000004, 0x01000005, 0x01000006, 0x01000007, 0x01000008, 0x01000009, 0x0100000A, 0x0100000B, 0x0100000C, 0x0100000D, 0x0100000E, 0x0100000F, 0x01000010, 0x02000001}}, {0x0200000B, 0x3F101, {0x01000001, 0x01000002, 0x01000003, 0x01000004, 0x01000005, 0x01000006, 0x01000007, 0x01000008, 0x01000009, 0x0100000A, 0x0100000B, 0x0100000C, 0x0100000D, 0x0100000E, 0x0100000F, 0x01000010, 0x02000001}}, {0x0200000C, 0x3F201, {0x01000001, 0x01000002, 0x01000003, 0x01000004, 0x01000005, 0x01000006, 0x01000007, 0x01000008, 0x01000009, 0x0100000A, 0x0100000B, 0x0100000C, 0x0100000D, 0x0100000E, 0x0100000F, 0x01000010, 0x02000001}}, {0x0200000D, 0x3F301, {0x01000001, 0x01000002, 0x01000003, 0x01000004, 0x01000005, 0x01000006, 0x01000007, 0x01000008, 0x01000009, 0x0100000A, 0x0100000B, 0x0100000C, 0x0100000D, 0x0100000E, 0x0100000F, 0x01000010, 0x02000001}}, {0x0200000E, 0x3F401, {0x01000001, 0x01000002, 0x01000003, 0x01000004, 0x01000005, 0x01000006, 0x01000007, 0x01000008, 0x01000009, 0x0100000A, 0x0100000B, 0x0100000C, 0x0100000D, 0x0100000E, 0x0100000F, 0x01000010, 0x02000001}}, {0x0200000F, 0x3F501, {0x01000001, 0x01000002, 0x01000003, 0x01000004, 0x01000005, 0x01000006, 0x01000007, 0x01000008, 0x01000009, 0x0100000A, 0x0100000B, 0x0100000C, 0x0100000D, 0x0100000E, 0x0100000F, 0x01000010, 0x02000001}}, {0x02000010, 0x3F601, {0x01000001, 0x01000002, 0x01000003, 0x01000004, 0x01000005, 0x01000006, 0x01000007, 0x01000008, 0x01000009, 0x0100000A, 0x0100000B, 0x0100000C, 0x0100000D, 0x0100000E, 0x0100000F, 0x01000010, 0x02000001}}, {0x01000010, 0x1101, {0x0100000F}}, {0x0100000F, 0x1001, {0x0100000E}}, {0x0100000E, 0xF01, {0x0100000D}}, {0x0100000D, 0xE01, {0x0100000C}}, {0x0100000C, 0xD01, {0x0100000B}}, {0x0100000B, 0xC01, {0x0100000A}}, {0x0100000A, 0xB01, {0x01000009}}, {0x01000009, 0xA01, {0x01000008}}, {0x01000008, 0x901, {0x01000007}}, {0x01000007, 0x801, {0x01000006}}, {0x01000006, 0x701, {0x01000005}}, {0x01000005, 0x601, {0x01000004}}, {0x01000004, 0x501, {0x01000003}}, {0x01000003, 0x401, {0x01000002}}, {0x01000002, 0x301, {0x01000001}}, {0x01000001, 0x201, {}}},
   {31, 30, 29, 28, 27, 26, 25, 24, 23, 22, 21, 20, 19, 18, 17, 16},
   {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 31, 31, 31, 31, 31, 31, 31, 31, 31, 31, 31, 31, 31, 31, 31, 31}},
  {"lists exceed", 2, 17, 32, 2, 16,
   {{0x02000001, 0x102, {0x0200FFFF}}, {0x02000002, 0x3E801, {0x01000001, 0x01000002, 0x01000003, 0x01000004, 0x01000005, 0x01000006, 0x01000007, 0x01000008, 0x01000009, 0x0100000A, 0x0100000B, 0x0100000C, 0x0100000D, 0x0100000E, 0x0100000F, 0x01000010, 0x02000001}}, {0x02000003, 0x3E901, {0x01000001, 0x01000002, 0x01000003, 0x01000004, 0x01000005, 0x01000006, 0x01000007, 0x01000008, 0x01000009, 0x0100000A, 0x0100000B, 0x0100000C, 0x0100000D, 0x0100000E, 0x0100000F, 0x01000010, 0x02000001}}, {0x02000004, 0x3EA01, {0x01000001, 0x01000002, 0x01000003, 0x01000004, 0x01000005, 0x01000006, 0x01000007, 0x01000008, 0x01000009, 0x0100000A, 0x0100000B, 0x0100000C, 0x0100000D, 0x0100000E, 0x0100000F, 0x01000010, 0x02000001}}, {0x02000005, 0x3EB01, {0x01000001, 0x01000002, 0x01000003, 0x01000004, 0x01000005, 0x01000006, 0x01000007, 0x01000008, 0x01000009, 0x0100000A, 0x0100000B, 0x0100000C, 0x0100000D, 0x0100000E, 0x0100000F, 0x01000010, 0x02000001}}, {0x02000006, 0x3EC01, {0x01000001, 0x01000002, 0x01000003, 0x01000004, 0x01000005, 0x01000006, 0x01000007, 0x01000008, 0x01000009, 0x0100000A, 0x0100000B, 0x0100000C, 0x0100000D, 0x0100000E, 0x0100000F, 0x01000010, 0x02000001}}, {0x02000007, 0x3ED01, {0x01000001, 0x01000002, 0x01000003, 0x01000004, 0x01000005, 0x01000006, 0x01000007, 0x01000008, 0x01000009, 0x0100000A, 0x0100000B, 0x0100000C, 0x0100000D, 0x0100000E, 0x0100000F, 0x01000010, 0x02000001}}, {0x02000008, 0x3EE01, {0x01000001, 0x01000002, 0x01000003, 0x01000004, 0x01000005, 0x01000006, 0x01000007, 0x01000008, 0x01000009, 0x0100000A, 0x0100000B, 0x0100000C, 0x0100000D, 0x0100000E, 0x0100000F, 0x01000010, 0x02000001}}, {0x02000009, 0x3EF01, {0x01000001, 0x01000002, 0x01000003, 0x01000004, 0x01000005, 0x01000006, 0x01000007, 0x01000008, 0x01000009, 0x0100000A, 0x0100000B, 0x0100000C, 0x0100000D, 0x0100000E, 0x0100000F, 0x01000010, 0x02000001}}, {0x0200000A, 0x3F001, {0x01000001, 0x01000002, 0x01000003, 0x01000004, 0x01000005, 0x01000006, 0x01000007, 0x01000008, 0x01000009, 0x0100000A, 0x0100000B, 0x0100000C, 0x0100000D, 0x0100000E, 0x0100000F, 0x01000010, 0x02000001}}, {0x0200000B, 0x3F101, {0x01000001, 0x01000002, 0x01000003, 0x01000004, 0x01000005, 0x01000006, 0x01000007, 0x01000008, 0x01000009, 0x0100000A, 0x0100000B, 0x0100000C, 0x0100000D, 0x0100000E, 0x0100000F, 0x01000010, 0x02000001}}, {0x0200000C, 0x3F201, {0x01000001, 0x01000002, 0x01000003, 0x01000004, 0x01000005, 0x01000006, 0x01000007, 0x01000008, 0x01000009, 0x0100000A, 0x0100000B, 0x0100000C, 0x0100000D, 0x0100000E, 0x0100000F, 0x01000010, 0x02000001}}, {0x0200000D, 0x3F301, {0x01000001, 0x01000002, 0x01000003, 0x01000004, 0x01000005, 0x01000006, 0x01000007, 0x01000008, 0x01000009, 0x0100000A, 0x0100000B, 0x0100000C, 0x0100000D, 0x0100000E, 0x0100000F, 0x01000010, 0x02000001}}, {0x0200000E, 0x3F401, {0x01000001, 0x01000002, 0x01000003, 0x01000004, 0x01000005, 0x01000006, 0x01000007, 0x01000008, 0x01000009, 0x0100000A, 0x0100000B, 0x0100000C, 0x0100000D, 0x0100000E, 0x0100000F, 0x01000010, 0x02000001}}, {0x0200000F, 0x3F501, {0x01000001, 0x01000002, 0x01000003, 0x01000004, 0x01000005, 0x01000006, 0x01000007, 0x01000008, 0x01000009, 0x0100000A, 0x0100000B, 0x0100000C, 0x0100000D, 0x0100000E, 0x0100000F, 0x01000010, 0x02000001}}, {0x02000010, 0x3F601, {0x01000001, 0x01000002, 0x01000003, 0x01000004, 0x01000005, 0x01000006, 0x01000007, 0x01000008, 0x01000009, 0x0100000A, 0x0100000B, 0x0100000C, 0x0100000D, 0x0100000E, 0x0100000F, 0x01000010, 0x02000001}}, {0x02000011, 0x3F701, {0x01000001, 0x01000002, 0x01000003, 0x01000004, 0x01000005, 0x01000006, 0x01000007, 0x01000008, 0x01000009, 0x0100000A, 0x0100000B, 0x0100000C, 0x0100000D, 0x0100000E, 0x0100000F, 0x01000010, 0x02000001}}, {0x01000010, 0x1101, {0x0100000F}}, {0x0100000F, 0x1001, {0x0100000E}}, {0x0100000E, 0xF01, {0x0100000D}}, {0x0100000D, 0xE01, {0x0100000C}}, {0x0100000C, 0xD01, {0x0100000B}}, {0x0100000B, 0xC01, {0x0100000A}}, {0x0100000A, 0xB01, {0x01000009}}, {0x01000009, 0xA01, {0x01000008}}, {0x01000008, 0x901, {0x01000007}}, {0x01000007, 0x801, {0x01000006}}, {0x01000006, 0x701, {0x01000005}}, {0x01000005, 0x601, {0x01000004}}, {0x01000004, 0x501, {0x01000003}}, {0x01000003, 0x401, {0x01000002}}, {0x01000002, 0x301, {0x01000001}}, {0x01000001, 0x201, {}}},
   {32, 31, 30, 29, 28, 27, 26, 25, 24, 23, 22, 21, 20, 19, 18, 17},
   {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32}},
};

struct Out {
  std::vector<uint32_t> order, release, nexec, err;
  fx_order_batch b;
  Out(uint32_t S, uint32_t steps)
      : order(fx_plane_words(S, steps), A5), release(fx_plane_words(S, steps), A5), nexec(S, A5), err(S, A5) {
    b = fx_order_batch{order.data(), release.data(), nexec.data(), err.data()};
  }
  bool operator==(const Out& o) const {
    return order == o.order && release == o.release && nexec == o.nexec && err == o.err;
  }
};

// a session over one stream in lane `lane` of S lanes (the others stay empty)
struct Session {
  const Stream& st;
  uint32_t S, lane, steps, tier, flags;
  std::vector<uint32_t> dot, hdr, deps, clo, chi, nd, lengths;
  std::vector<unsigned char> state;
  Out out;
  Session(const Stream& st_, uint32_t S_ = 3, uint32_t lane_ = 1, uint32_t tier_ = FX_PRED_TIER_SMALL, uint32_t flags_ = 0)
      : st(st_), S(S_), lane(lane_), steps((uint32_t)st_.rows.size()), tier(tier_), flags(flags_),
        dot(fx_plane_words(S, steps), A5), hdr(dot.size(), A5), deps(dot.size() * st.dmax, A5), clo(dot.size(), A5),
        chi(dot.size(), A5), nd(dot.size(), A5), lengths(S, 0u),
        state(fx_pred_session_bytes(tier, st.n, st.dmax, S), 0xA5), out(S, steps) {
    for (uint32_t r = 0; r < steps; ++r) {
      const size_t at = fx_index(r, lane, steps);
      const Row& row = st.rows[r];
      dot[at] = row.dot;
      hdr[at] = 9u * r;
      clo[at] = (uint32_t)row.clock;
      chi[at] = (uint32_t)(row.clock >> 32);
      nd[at] = (uint32_t)row.deps.size();
      for (uint32_t j = 0; j < row.deps.size(); ++j) deps[(size_t)j * dot.size() + at] = row.deps[j];
    }
  }
  fx_pred_batch batch(uint32_t call_steps = 0) const {
    fx_pred_batch in{};
    in.base = fx_stream_batch{dot.data(), hdr.data(), deps.data(), lengths.data(), S, call_steps ? call_steps : steps,
                              st.dmax, st.n};
    in.clock_lo = clo.data();
    in.clock_hi = chi.data();
    in.ndeps = nd.data();
    return in;
  }
  int advance(uint32_t len, bool init, uint32_t call_steps = 0) {
    lengths[lane] = len;
    const fx_pred_batch in = batch(call_steps);
    return fx_pred_advance_host(&in, &out.b, tier, state.data(), flags | (init ? FX_FLAG_INIT : 0u));
  }
  // a fresh one-call session with the same lengths
  void check_against_one_call(const char* what, uint32_t call) {
    Session whole(st, S, lane, tier, flags);
    EXPECT(whole.advance(lengths[lane], true) == FX_OK, "%s: the one-call session", st.name);
    EXPECT(out == whole.out, "%s, %s: call %u differs from one call", st.name, what, call);
  }
  // what the stream leaves when it is handed over whole, written out above
  void check_final(const char* what) {
    Out want(S, steps);
    for (uint32_t s = 0; s < S; ++s) want.nexec[s] = want.err[s] = 0;
    want.nexec[lane] = st.nexec;
    want.err[lane] = st.err;
    for (uint32_t k = 0; k < st.order.size(); ++k) want.order[fx_index(k, lane, steps)] = st.order[k] | FX_ORDER_SCC_START;
    for (uint32_t r = 0; r < st.release.size(); ++r)
      if (st.release[r] >= 0) want.release[fx_index(r, lane, steps)] = (uint32_t)st.release[r];
    EXPECT(st.order.size() == st.nexec, "%s: the expectation itself", st.name);
    EXPECT(out == want, "%s, %s: differs from what is written out", st.name, what);
  }
};

void run_cuts(const Stream& st, const char* what, const std::vector<uint32_t>& cuts) {
  Session x(st);
  for (uint32_t c = 0; c < cuts.size(); ++c) {
    EXPECT(x.advance(std::min<uint32_t>(cuts[c], x.steps), c == 0) == FX_OK, "%s, %s: call %u", st.name, what, c);
    x.check_against_one_call(what, c);
  }
  x.check_final(what);
}

}  // namespace

int main() {
  for (const Stream& st : STREAMS) {
    const uint32_t L = (uint32_t)st.rows.size();
    run_cuts(st, "whole", {L});
    run_cuts(st, "cut before the last or failing row", {st.cut, L});
    std::vector<uint32_t> rows;
    for (uint32_t r = 0; r <= L; ++r) rows.push_back(r);
    run_cuts(st, "a row per call", rows);
    run_cuts(st, "untouched twice, then whole", {0, 0, L});
    run_cuts(st, "larger lengths behind the end", {st.cut, L, L + 1, L + 50});
  }
  {
    const Stream& st = STREAMS[0];
    // a state that never saw FX_FLAG_INIT
    Session x(st);
    const std::vector<unsigned char> raw = x.state;
    EXPECT(x.advance(4, false) == FX_OK, "a call on a raw state");
    EXPECT(x.out.err[0] == FX_ERR_INVALID_ARG && x.out.err[1] == FX_ERR_INVALID_ARG && x.out.err[2] == FX_ERR_INVALID_ARG,
           "a raw state accepted");
    EXPECT(x.out.nexec[1] == A5 && x.out.order == Out(x.S, x.steps).order && x.out.release == Out(x.S, x.steps).release &&
               x.state == raw,
           "a call on a raw state wrote");
    EXPECT(x.advance(3, true) == FX_OK, "init");
    x.check_against_one_call("contract", 0);
    const std::vector<unsigned char> kept = x.state;
    const Out before = x.out;
    // other steps, the other commit flag, another tier, dmax one more, the ndeps plane dropped
    EXPECT(x.advance(4, false, 3) == FX_OK && x.out.err[1] == FX_ERR_INVALID_ARG && x.state == kept, "other steps");
    x.flags = FX_FLAG_EXECUTE_AT_COMMIT;
    EXPECT(x.advance(4, false) == FX_OK && x.out.err[1] == FX_ERR_INVALID_ARG && x.state == kept, "other commit flag");
    x.flags = 0;
    x.tier = FX_PRED_TIER_LDS;
    EXPECT(x.advance(4, false) == FX_OK && x.out.err[1] == FX_ERR_INVALID_ARG && x.state == kept, "another tier");
    x.tier = FX_PRED_TIER_SMALL;
    {
      x.lengths[x.lane] = 4;
      fx_pred_batch in = x.batch();
      in.base.dmax += 1;
      EXPECT(fx_pred_advance_host(&in, &x.out.b, x.tier, x.state.data(), 0) == FX_OK && x.out.err[1] == FX_ERR_INVALID_ARG &&
                 x.state == kept,
             "dmax one more");
      in = x.batch();
      in.ndeps = nullptr;
      EXPECT(fx_pred_advance_host(&in, &x.out.b, x.tier, x.state.data(), 0) == FX_OK && x.out.err[1] == FX_ERR_INVALID_ARG &&
                 x.state == kept,
             "the ndeps plane dropped");
    }
    // len < done, then the rest
    EXPECT(x.advance(2, false) == FX_OK && x.out.err[1] == FX_ERR_INVALID_ARG && x.out.nexec[1] == 0 && x.state == kept,
           "a shorter length");
    EXPECT(x.out.order == before.order && x.out.release == before.release && x.out.nexec == before.nexec,
           "a refused stream wrote more than err");
    EXPECT(x.advance(4, false) == FX_OK, "the rest");
    x.check_final("behind the refused calls");
    // refusals
    fx_pred_batch in = x.batch();
    const Out out_before = x.out;
    const std::vector<unsigned char> state_before = x.state;
    EXPECT(fx_pred_advance_host(&in, &x.out.b, 0, nullptr, FX_FLAG_INIT) == FX_ERR_INVALID_ARG, "a null state accepted");
    EXPECT(fx_pred_advance_host(nullptr, &x.out.b, 0, x.state.data(), 0) == FX_ERR_INVALID_ARG, "a null batch accepted");
    EXPECT(fx_pred_advance_host(&in, nullptr, 0, x.state.data(), 0) == FX_ERR_INVALID_ARG, "a null out accepted");
    EXPECT(fx_pred_advance_host(&in, &x.out.b, 3, x.state.data(), 0) == FX_ERR_INVALID_ARG, "tier 3 accepted");
    EXPECT(fx_pred_advance_host(&in, &x.out.b, 0, x.state.data(), FX_FLAG_SAVE_STATE) == FX_ERR_INVALID_ARG,
           "an unknown flag accepted");
    in.base.steps = 1u << 26;
    EXPECT(fx_pred_advance_host(&in, &x.out.b, 0, x.state.data(), 0) == FX_ERR_INVALID_ARG, "steps 2^26 accepted");
    in = x.batch();
    in.clock_lo = nullptr;
    EXPECT(fx_pred_advance_host(&in, &x.out.b, 0, x.state.data(), 0) == FX_ERR_INVALID_ARG, "a null plane accepted");
    in = x.batch();
    in.base.n = 9;
    EXPECT(fx_pred_advance_host(&in, &x.out.b, 0, x.state.data(), 0) == FX_ERR_INVALID_ARG, "n = 9 accepted");
    EXPECT(x.out == out_before && x.state == state_before, "a refused call wrote");
    EXPECT(fx_pred_session_bytes(FX_PRED_TIER_SMALL, 5, 5, 2) == 2u * (16u + 1152u) * 4u, "session bytes");
    EXPECT(fx_pred_session_bytes(3, 5, 5, 2) == 0u, "session bytes of tier 3");
  }
  {
    // every tier, and the compiled SMALL layout, over the base stream a row per call
    Stream five = STREAMS[0];
    five.n = 5;
    five.dmax = 5;
    for (uint32_t tier = FX_PRED_TIER_SMALL; tier <= FX_PRED_TIER_HBM; ++tier)
      for (const Stream* st : {&STREAMS[0], (const Stream*)&five}) {
        Session x(*st, 2, 0, tier);
        for (uint32_t r = 0; r <= x.steps; ++r) EXPECT(x.advance(r, r == 0) == FX_OK, "tier %u, row %u", tier, r);
        x.check_final("every tier");
      }
  }
  if (failures) {
    printf("%d checks failed\n", failures);
    return 1;
  }
  printf("pred_advance_host_check: ok\n");
  return 0;
}
