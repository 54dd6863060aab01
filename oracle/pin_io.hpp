/*
 * pin_io.hpp -- TEST INFRASTRUCTURE: what the programs of the reference-frame pin share and what
 * does not depend on a header set: float32 arrays as .npy files and the words of the index of cases.
 */
#pragma once

#include <cstdio>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace PinIO {

/* NumPy format 1.0, little endian float32, C order */
inline bool writeNpy(const std::string& fileName, const std::vector<size_t>& shape, const float* data)
{
    std::string dict = "{'descr': '<f4', 'fortran_order': False, 'shape': (";
    size_t count = 1;
    for (size_t d : shape) {
        dict += std::to_string(d) + ",";
        count *= d;
    }
    dict += "), }";
    while ((10 + dict.size() + 1) % 64 != 0)
        dict += ' ';
    dict += '\n';
    FILE* f = fopen(fileName.c_str(), "wb");
    if (!f)
        return false;
    const unsigned char head[10] = { 0x93, 'N', 'U', 'M', 'P', 'Y', 1, 0, (unsigned char)(dict.size() & 0xff), (unsigned char)(dict.size() >> 8) };
    bool ok = fwrite(head, 1, 10, f) == 10 && fwrite(dict.data(), 1, dict.size(), f) == dict.size()
        && fwrite(data, sizeof(float), count, f) == count;
    return fclose(f) == 0 && ok;
}

/* the float32 rows of a .npy file written by PinIO::writeNpy */
inline bool readRows(const std::string& fileName, size_t width, std::vector<float>& rows)
{
    FILE* f = fopen(fileName.c_str(), "rb");
    if (!f)
        return false;
    unsigned char head[10];
    bool ok = fread(head, 1, 10, f) == 10 && memcmp(head, "\x93NUMPY", 6) == 0;
    if (ok) {
        const long dict = head[8] | (head[9] << 8);
        ok = fseek(f, 0, SEEK_END) == 0;
        const long size = ftell(f);
        ok = ok && size >= 10 + dict && (size - 10 - dict) % long(width * sizeof(float)) == 0 && fseek(f, 10 + dict, SEEK_SET) == 0;
        if (ok) {
            rows.resize((size - 10 - dict) / sizeof(float));
            ok = fread(rows.data(), sizeof(float), rows.size(), f) == rows.size();
        }
    }
    fclose(f);
    return ok;
}

inline std::string jsonList(const char* words)
{
    std::string r = "[", w;
    bool first = true;
    for (const char* p = words;; p++) {
        if (*p == ' ' || *p == 0) {
            if (!w.empty()) {
                r += std::string(first ? "" : ", ") + "\"" + w + "\"";
                first = false;
                w.clear();
            }
            if (*p == 0)
                break;
        } else {
            w += *p;
        }
    }
    return r + "]";
}

}
