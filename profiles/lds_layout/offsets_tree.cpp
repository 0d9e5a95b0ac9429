#include "mrts_engine.hip"
#include "offsets_common.h"
int main() {
    using namespace mrts;
    unsigned char* z = lds_any_base();
    for (int w = 1; w <= 48; w++) for (int h = 1; h <= 64; h++) for (int NT = 64; NT <= 256; NT *= 2) {
        const int HW = w * h;
        printf("%d %d %d U", w, h, NT);
        Carver c{z}; Lds U = carve(c, HW, w, NT); LDS(U); printf(" %zu", c.o);
        printf(" K"); size_t kb; bots::BL K = bots::bot_carve(z, HW, w, &kb); BLL(K); printf(" %zu\n", kb);
        for (int early = 0; early < 2; early++) for (int botg = 0; botg < 2; botg++) {
            printf("%d %d %d F%d%d", w, h, NT, early, botg);
            FusedLds F = fused_carve(z, HW, w, NT, early, botg);
            LDS(F.L); BLL(F.B); O(F.tail); printf(" %zu", (size_t)F.tail_words); O(F.early_cnt);
            printf(" %zu\n", F.bytes);
        }
    }
}
