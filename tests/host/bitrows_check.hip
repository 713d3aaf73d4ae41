// Host program of tests/test_bit_rows_host.py: for every 96-bit payload word of the input file, the Tx batch's bit
// rows 3..9 as the kernels build them (ofdm_rxcommon.h demap_word<0..3>, pair_words: two-bit field moves) and as
// the reference loops state them (demap_word_ref, pair_words_ref: a bit at a time).  Compiled for the host only;
// it makes no HIP call.
// usage: bitrows_check in.bin out.bin   (in: n x 3 uint32; out: n x 14 uint32, 7 built words then 7 stated ones)
#include <cstdio>
#include <vector>
#include "ofdm_rxcommon.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *fi = fopen(argv[1], "rb");
    if (!fi) return 2;
    std::vector<uint32_t> in;
    uint32_t w[3];
    while (fread(w, sizeof(uint32_t), 3, fi) == 3) in.insert(in.end(), w, w + 3);
    fclose(fi);
    std::vector<uint32_t> out;
    out.reserve(in.size() / 3 * 14);
    for (size_t i = 0; i + 3 <= in.size(); i += 3) {
        const uint32_t *p = &in[i];
        uint32_t t[4], pw[3];
        ofdm::demap_words(p, t);
        ofdm::pair_words(p, pw);
        out.insert(out.end(), t, t + 4);
        out.insert(out.end(), pw, pw + 3);
        const uint32_t r[4] = {ofdm::demap_word_ref<0>(p), ofdm::demap_word_ref<1>(p), ofdm::demap_word_ref<2>(p),
                               ofdm::demap_word_ref<3>(p)};
        ofdm::pair_words_ref(p, pw);
        out.insert(out.end(), r, r + 4);
        out.insert(out.end(), pw, pw + 3);
    }
    FILE *fo = fopen(argv[2], "wb");
    if (!fo) return 2;
    const bool ok = fwrite(out.data(), sizeof(uint32_t), out.size(), fo) == out.size();
    return fclose(fo) == 0 && ok ? 0 : 2;
}
