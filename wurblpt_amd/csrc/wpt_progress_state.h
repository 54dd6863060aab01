/*
 * wpt_progress_state.h -- the header of a saved progressive session (include/wurblpt_hip.h, wpt_progress_save): its layout
 * and the parser that wpt_progress_state_info and wpt_progress_restore use.  Plain host C++ without a HIP include, so that
 * it also compiles outside the library (tests/progress_state_check.cpp runs it under the sanitizers).
 *
 * The parser reads a byte only after it has checked that the byte lies within `bytes`, and it reads the buffer with memcpy:
 * the buffer needs no alignment.  All words are little-endian, which is the byte order of every host the library runs on.
 */
#ifndef WPT_PROGRESS_STATE_H
#define WPT_PROGRESS_STATE_H

#include <stdint.h>
#include <stddef.h>
#include <string.h>

#include "../../include/wurblpt_hip.h"

namespace wptp {

/* byte offsets of the header's fields (wurblpt_hip.h has the table) */
enum : size_t {
    STATE_MAGIC = 0,
    STATE_VERSION = 4,
    STATE_WIDTH = 8,
    STATE_HEIGHT = 12,
    STATE_SAMPLES_SQRT = 16,
    STATE_BLOCK_START = 20,
    STATE_BLOCK_SIZE = 24,
    STATE_ROWS_DONE = 28,
    STATE_TAG = 32,
    STATE_CAMERA = 40,
    STATE_PARAMS = STATE_CAMERA + sizeof(wpt_camera),
    STATE_RESERVED = STATE_PARAMS + sizeof(wpt_params),
    STATE_HEADER_BYTES = STATE_RESERVED + 4
};
static_assert(STATE_HEADER_BYTES == WPT_PROGRESS_HEADER_BYTES, "the header's size is part of the ABI");
static_assert(STATE_HEADER_BYTES % 16 == 0, "the carry quadwords start on a multiple of 16 bytes");
constexpr size_t STATE_CARRY_BYTES_PER_PIXEL = 32;

struct StateField {
    const char* name;
    size_t offset, bytes;
    const char* cut; /* the message of a state that ends within this field */
};
static const StateField STATE_FIELDS[] = {
    { "magic", STATE_MAGIC, 4, "the state ends within its magic" },
    { "version", STATE_VERSION, 4, "the state ends within its version" },
    { "width", STATE_WIDTH, 4, "the state ends within width" },
    { "height", STATE_HEIGHT, 4, "the state ends within height" },
    { "samples_sqrt", STATE_SAMPLES_SQRT, 4, "the state ends within samples_sqrt" },
    { "block_start", STATE_BLOCK_START, 4, "the state ends within block_start" },
    { "block_size", STATE_BLOCK_SIZE, 4, "the state ends within block_size" },
    { "rows_done", STATE_ROWS_DONE, 4, "the state ends within rows_done" },
    { "tag", STATE_TAG, 8, "the state ends within tag" },
    { "camera", STATE_CAMERA, sizeof(wpt_camera), "the state ends within camera" },
    { "params", STATE_PARAMS, sizeof(wpt_params), "the state ends within params" },
    { "reserved", STATE_RESERVED, 4, "the state ends within its reserved word" },
};

inline uint32_t stateWord(const void* buffer, size_t offset)
{
    uint32_t v;
    memcpy(&v, static_cast<const unsigned char*>(buffer) + offset, sizeof(v));
    return v;
}

inline void statePutWord(void* buffer, size_t offset, uint32_t v)
{
    memcpy(static_cast<unsigned char*>(buffer) + offset, &v, sizeof(v));
}

/* Checks a state of `bytes` bytes and fills `info`.  NULL: the state is good; otherwise the reason it is refused for, a string
 * constant.  Nothing at or behind buffer + bytes is read. */
inline const char* parseState(const void* buffer, size_t bytes, wpt_progress_info* info)
{
    if (!buffer)
        return "the state is NULL";
    for (const StateField& f : STATE_FIELDS)
        if (bytes < f.offset + f.bytes)
            return f.cut;
    if (stateWord(buffer, STATE_MAGIC) != WPT_PROGRESS_MAGIC)
        return "not a saved session: wrong magic";
    wpt_progress_info i;
    memset(&i, 0, sizeof(i));
    i.version = stateWord(buffer, STATE_VERSION);
    if (i.version != WPT_PROGRESS_STATE_VERSION)
        return "the state's format version is not this library's";
    i.width = stateWord(buffer, STATE_WIDTH);
    i.height = stateWord(buffer, STATE_HEIGHT);
    i.samples_sqrt = stateWord(buffer, STATE_SAMPLES_SQRT);
    i.block_start = stateWord(buffer, STATE_BLOCK_START);
    i.block_size = stateWord(buffer, STATE_BLOCK_SIZE);
    i.rows_done = stateWord(buffer, STATE_ROWS_DONE);
    memcpy(&i.tag, static_cast<const unsigned char*>(buffer) + STATE_TAG, sizeof(i.tag));
    if (i.width == 0 || i.height == 0 || i.samples_sqrt == 0 || i.width > 65535 || i.height > 65535 || i.samples_sqrt > 65535)
        return "the state's width, height and samples_sqrt must lie in 1 .. 65535";
    if (i.block_size == 0 || uint64_t(i.block_start) + i.block_size > uint64_t(i.width) * i.height)
        return "the state's block lies outside width * height";
    if (i.rows_done > i.samples_sqrt)
        return "the state's rows_done is greater than its samples_sqrt";
    i.state_bytes = uint64_t(STATE_HEADER_BYTES) + uint64_t(i.block_size) * STATE_CARRY_BYTES_PER_PIXEL;
    if (stateWord(buffer, STATE_RESERVED) != 0)
        return "the state's reserved word is not 0";
    if (uint64_t(bytes) < i.state_bytes)
        return "the state ends within its carry";
    if (uint64_t(bytes) > i.state_bytes)
        return "the state is longer than its header says";
    if (info)
        *info = i;
    return nullptr;
}

/* The first record of a parsed state whose next stratum is not i = 0 of row rows_done, which is where every pixel of a saved
 * session stands (a session without a stage holds zeros, which says the same); info.block_size if all records do. */
inline uint64_t firstDamagedRecord(const void* buffer, const wpt_progress_info& info)
{
    for (uint64_t k = 0; k < info.block_size; k++)
        if (stateWord(buffer, STATE_HEADER_BYTES + size_t(k) * STATE_CARRY_BYTES_PER_PIXEL + 28) != info.rows_done << 16)
            return k;
    return info.block_size;
}

/* writes the header of a state into buffer[0 .. STATE_HEADER_BYTES) */
inline void writeStateHeader(void* buffer, const wpt_progress_info& i, const wpt_camera& camera, const wpt_params& params)
{
    unsigned char* b = static_cast<unsigned char*>(buffer);
    memset(b, 0, STATE_HEADER_BYTES);
    statePutWord(b, STATE_MAGIC, WPT_PROGRESS_MAGIC);
    statePutWord(b, STATE_VERSION, WPT_PROGRESS_STATE_VERSION);
    statePutWord(b, STATE_WIDTH, i.width);
    statePutWord(b, STATE_HEIGHT, i.height);
    statePutWord(b, STATE_SAMPLES_SQRT, i.samples_sqrt);
    statePutWord(b, STATE_BLOCK_START, i.block_start);
    statePutWord(b, STATE_BLOCK_SIZE, i.block_size);
    statePutWord(b, STATE_ROWS_DONE, i.rows_done);
    memcpy(b + STATE_TAG, &i.tag, sizeof(i.tag));
    memcpy(b + STATE_CAMERA, &camera, sizeof(camera));
    memcpy(b + STATE_PARAMS, &params, sizeof(params));
}

} /* namespace wptp */

#endif
