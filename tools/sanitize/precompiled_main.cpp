// precompiled_main.cpp -- a stand-alone driver for the Precompiled normalizer's reader of untrusted bytes (host/precompiled.h), meant
// to be built with -fsanitize=address,undefined and run on the CPU:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/sanitize/precompiled_main.cpp -o /tmp/precompiled_san
//   /tmp/precompiled_san tests/golden/nmt_nfkc_charsmap.bin
//
// It feeds the reader the character map whole, cut at many lengths, with its header and single trie units overwritten, and a few
// hand-made maps, and normalises a line of every script the tests name with each map that loads.  Every malformed map must end in a
// semtools::Error; the sanitizers see every read.  Prints what it counted; exit status 0 unless something else was thrown.
#include <cstdio>
#include <fstream>
#include <iterator>

#include "../../semtools_amd/csrc/host/precompiled.h"

using semtools::Error;
using semtools::PrecompiledMap;

static const char32_t *TEXTS[] = {U"ﬁne  Straße ｆｕｌｌ  x² ｶﾞ é Ⅻ №5​ 한글",
                                  U"a \U0001F468‍\U0001F469‍\U0001F467 \U0001F1E9\U0001F1EA 한 ½ ㍿ ﷺ \r\n\tक्ष",
                                  U"", U"a", U"the quick fox"};

static int loaded = 0, refused_at_load = 0, refused_at_lookup = 0;

static void feed(const std::string &blob)
{
    bool is_loaded = false;
    try {
        const PrecompiledMap map(blob);
        is_loaded = true;
        std::u32string out;
        for (const char32_t *t : TEXTS) map.normalize(std::u32string(t), out);
        ++loaded;
    } catch (const Error &) {
        ++(is_loaded ? refused_at_lookup : refused_at_load);
    }
}

int main(int argc, char **argv)
{
    std::string blob;
    if (argc > 1) {
        std::ifstream f(argv[1], std::ios::binary);
        blob.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    }
    feed(std::string());
    feed(std::string("\x01\x02", 2));
    feed(std::string("\x06\0\0\0aaaaaaaaaaaa", 16));
    feed(std::string("\0\0\x10\0aaaaaaaaaaaa", 16));
    feed(std::string("\x04\0\0\0\0\xA0\x0F\0x\0", 10));   // one unit whose offset leads outside the trie
    feed(std::string("\0\0\0\0", 4));                     // an empty trie, an empty pool
    if (!blob.empty()) {
        feed(blob);
        for (size_t n = 0; n < blob.size(); n += blob.size() / 257 + 1) feed(blob.substr(0, n));
        feed(blob.substr(0, blob.size() - 1));
        for (uint32_t size : {0u, 1u, 3u, 4u, 8u, 0x7FFFFFFCu, 0xFFFFFFFCu, 0xFFFFFFFFu, (uint32_t)blob.size() - 4, (uint32_t)blob.size()}) {
            std::string b = blob;
            for (int k = 0; k < 4; ++k) b[k] = (char)(size >> (8 * k));
            feed(b);
        }
        const size_t units = blob.size() >= 4 ? ((uint8_t)blob[0] | (uint8_t)blob[1] << 8 | (uint8_t)blob[2] << 16 | (size_t)(uint8_t)blob[3] << 24) / 4 : 0;
        for (size_t u = 0; u < units; u += units / 499 + 1)    // single units overwritten: offsets and values that lead anywhere
            for (uint32_t v : {0xFFFFFFFFu, 0x7FFFFFFFu, 0xFFFFFD00u, 0x000003FFu}) {
                std::string b = blob;
                for (int k = 0; k < 4; ++k) b[4 + 4 * u + k] = (char)(v >> (8 * k));
                feed(b);
            }
    }
    std::printf("maps that loaded and normalised: %d, refused at load: %d, refused at a lookup: %d\n", loaded, refused_at_load, refused_at_lookup);
    return 0;
}
