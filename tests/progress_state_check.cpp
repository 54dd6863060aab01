/* progress_state_check.cpp -- the parser of a saved progressive session (wurblpt_amd/csrc/wpt_progress_state.h) on its own,
 * built with -fsanitize=address,undefined by tests/test_progress_state.py and run as a program.  Every state it parses lies in
 * a heap block of exactly its length, so that a read at or behind buffer + bytes is a heap overflow the sanitizer reports.
 *   progress_state_check [corruptions [seed]]
 * Walks the documented cases (a good state, a state cut at every field boundary and one byte short of its carry, wrong magic,
 * wrong version, a block that overflows width * height, rows_done > samples_sqrt), then `corruptions` seeded damaged states.
 * Prints one line per documented case ("name: message") and a summary; exit status 1 if a case is not judged as it must be. */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../wurblpt_amd/csrc/wpt_progress_state.h"

using namespace wptp;

static int failures = 0;

/* parses a copy of the state that lies in a heap block of its own length */
static const char* parseExact(const std::vector<unsigned char>& state, size_t bytes, wpt_progress_info* info)
{
    unsigned char* block = static_cast<unsigned char*>(malloc(bytes ? bytes : 1));
    if (bytes)
        memcpy(block, state.data(), bytes);
    const char* refused = parseState(bytes ? block : block + 1, bytes, info);
    free(block);
    return refused;
}

static void expect(const char* name, const std::vector<unsigned char>& state, size_t bytes, const char* word)
{
    wpt_progress_info info;
    memset(&info, 0xee, sizeof(info));
    const char* refused = parseExact(state, bytes, &info);
    printf("%s: %s\n", name, refused ? refused : "good");
    const bool ok = word ? (refused && strstr(refused, word)) : !refused;
    if (!ok) {
        printf("  EXPECTED %s\n", word ? word : "a good state");
        failures++;
    }
    if (refused && info.version != 0xeeeeeeeeu) {
        printf("  a refused state must leave info alone\n");
        failures++;
    }
}

static std::vector<unsigned char> goodState(uint32_t width, uint32_t height, uint32_t samplesSqrt, uint32_t start, uint32_t size, uint32_t rows)
{
    wpt_progress_info i;
    memset(&i, 0, sizeof(i));
    i.width = width;
    i.height = height;
    i.samples_sqrt = samplesSqrt;
    i.block_start = start;
    i.block_size = size;
    i.rows_done = rows;
    i.tag = 0x0123456789abcdefull;
    wpt_camera cam;
    wpt_params par;
    memset(&cam, 0x11, sizeof(cam));
    memset(&par, 0x22, sizeof(par));
    std::vector<unsigned char> state(STATE_HEADER_BYTES + size_t(size) * STATE_CARRY_BYTES_PER_PIXEL, 0x33);
    writeStateHeader(state.data(), i, cam, par);
    return state;
}

int main(int argc, char* argv[])
{
    const unsigned int corruptions = argc > 1 ? atoi(argv[1]) : 4000;
    const unsigned int seed = argc > 2 ? atoi(argv[2]) : 1;
    const std::vector<unsigned char> good = goodState(7, 5, 6, 3, 29, 2);

    expect("good", good, good.size(), nullptr);
    {
        wpt_progress_info info;
        if (parseExact(good, good.size(), &info) || info.width != 7 || info.height != 5 || info.samples_sqrt != 6 || info.block_start != 3
                || info.block_size != 29 || info.rows_done != 2 || info.tag != 0x0123456789abcdefull || info.state_bytes != good.size()
                || info.version != WPT_PROGRESS_STATE_VERSION) {
            printf("  the good state's info is wrong\n");
            failures++;
        }
    }
    /* a state cut at a field's first byte or at its last ends within that field: each has its own message */
    for (const StateField& f : STATE_FIELDS) {
        expect((std::string("cut at the start of ") + f.name).c_str(), good, f.offset, f.cut);
        expect((std::string("cut at the last byte of ") + f.name).c_str(), good, f.offset + f.bytes - 1, f.cut);
    }
    expect("header only", good, STATE_HEADER_BYTES, "carry");
    expect("one byte short of its carry", good, good.size() - 1, "carry");
    {
        std::vector<unsigned char> longer = good;
        longer.push_back(0);
        expect("one byte too long", longer, longer.size(), "longer");
    }
    auto damaged = [&](size_t offset, uint32_t value) {
        std::vector<unsigned char> s = good;
        statePutWord(s.data(), offset, value);
        return s;
    };
    expect("wrong magic", damaged(STATE_MAGIC, 0x50545058u), good.size(), "magic");
    expect("wrong version", damaged(STATE_VERSION, WPT_PROGRESS_STATE_VERSION + 1), good.size(), "version");
    expect("width 0", damaged(STATE_WIDTH, 0), good.size(), "1 .. 65535");
    expect("samples_sqrt 65536", damaged(STATE_SAMPLES_SQRT, 65536), good.size(), "1 .. 65535");
    expect("block_size overflows width * height", damaged(STATE_BLOCK_SIZE, 33), good.size(), "block");
    expect("block_start + block_size wraps", damaged(STATE_BLOCK_START, 0xfffffff0u), good.size(), "block");
    expect("block_size 0", damaged(STATE_BLOCK_SIZE, 0), good.size(), "block");
    expect("rows_done greater than samples_sqrt", damaged(STATE_ROWS_DONE, 7), good.size(), "rows_done");
    expect("reserved word not 0", damaged(STATE_RESERVED, 1), good.size(), "reserved");
    expect("rows_done equal to samples_sqrt", damaged(STATE_ROWS_DONE, 6), good.size(), nullptr);
    {
        /* the body: every record of the good state above holds 0x33 bytes, none stands at row 2 */
        wpt_progress_info info;
        std::vector<unsigned char> body = good;
        if (parseState(body.data(), body.size(), &info) || firstDamagedRecord(body.data(), info) != 0) {
            printf("  record 0 of the filler state must be found damaged\n");
            failures++;
        }
        for (uint32_t k = 0; k < info.block_size; k++)
            statePutWord(body.data(), STATE_HEADER_BYTES + 32 * k + 28, 2u << 16);
        if (firstDamagedRecord(body.data(), info) != info.block_size) {
            printf("  records that stand at row rows_done are good\n");
            failures++;
        }
        statePutWord(body.data(), STATE_HEADER_BYTES + 32 * 17 + 28, (2u << 16) | 1u);
        if (firstDamagedRecord(body.data(), info) != 17) {
            printf("  record 17 must be found damaged\n");
            failures++;
        }
    }
    if (!parseState(nullptr, 100, nullptr)) {
        printf("  a NULL state must be refused\n");
        failures++;
    }

    /* seeded damage: words of the header replaced, bytes flipped, the state cut anywhere or padded.  Whatever the parser says,
     * it must say it without reading outside the block, and a state it accepts has exactly the length its header gives */
    std::mt19937 rng(seed);
    unsigned int accepted = 0;
    for (unsigned int n = 0; n < corruptions; n++) {
        std::vector<unsigned char> s = good;
        const unsigned int kind = rng() % 4;
        if (kind == 0) {
            static const uint32_t values[] = { 0, 1, 2, 29, 35, 36, 65535, 65536, 0x7fffffffu, 0x80000000u, 0xffffffffu };
            statePutWord(s.data(), 4 * (rng() % 8), values[rng() % (sizeof(values) / sizeof(values[0]))]);
        } else if (kind == 1) {
            for (unsigned int k = 0, flips = 1 + rng() % 4; k < flips; k++)
                s[rng() % STATE_HEADER_BYTES] ^= static_cast<unsigned char>(1u << (rng() % 8));
        } else if (kind == 2) {
            statePutWord(s.data(), 4 * (2 + rng() % 6), rng());
        }
        size_t bytes = s.size();
        if (rng() % 2)
            bytes = rng() % (s.size() + 1);
        else if (rng() % 8 == 0)
            s.resize(bytes = s.size() + 1 + rng() % 64, 0);
        wpt_progress_info info;
        const char* refused = parseExact(s, bytes, &info);
        if (!refused) {
            accepted++;
            if (info.state_bytes != bytes || uint64_t(info.block_start) + info.block_size > uint64_t(info.width) * info.height
                    || info.rows_done > info.samples_sqrt) {
                printf("  corruption %u was accepted with an inconsistent header\n", n);
                failures++;
            }
        }
    }
    printf("%u corruptions (seed %u): %u still good states, %d failures\n", corruptions, seed, accepted, failures);
    return failures ? 1 : 0;
}
