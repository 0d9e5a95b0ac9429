#include "mrts_engine.hip"
#include "offsets_common.h"
int main() {
    using namespace mrts;
    unsigned char* z = reinterpret_cast<unsigned char*>((size_t)1 << 20);
    for (int w = 1; w <= 48; w++) for (int h = 1; h <= 64; h++) for (int NT = 64; NT <= 256; NT *= 2) {
        const int HW = w * h;
        printf("%d %d %d U", w, h, NT);
        Lds U = carve(z, HW, w, NT); LDS(U); printf(" %zu", lds_bytes(HW, w, NT));
        printf(" K"); bots::BL K = bots::bot_carve(z, HW, w); BLL(K); printf(" %zu\n", bots::bot_lds_bytes(HW, w));
        for (int early = 0; early < 2; early++) for (int botg = 0; botg < 2; botg++) {
            printf("%d %d %d F%d%d", w, h, NT, early, botg);
            Lds L = carve(z, HW, w, NT, false, z + fb_wall_offset(HW, w, NT, early));
            if (botg) { uint32_t* region = (uint32_t*)(z + fb_outw_offset(HW, w, NT)); L.outw = early ? (uint32_t*)L.uid : region; L.outm = early ? region : region + HW; }
            unsigned char* tail = z + fb_tail_offset(HW, w, NT, early);
            bots::BL B = bots::bot_carve(z, HW, w, tail, false); B.wall = L.wall;
            LDS(L); BLL(B); O(tail); printf(" %zu", bots::bot_tail_bytes(HW, w) / 4); O(z + fb_early_cnt_offset(HW, w, NT, early));
            printf(" %zu\n", fb_lds_bytes(HW, w, NT, early));
        }
    }
}
