#include <cstdio>
#define O(p) printf(" %ld", (long)((const unsigned char*)(p) - z))
#define LDS(L) O(L.unit);O(L.uid);O(L.act);O(L.seq);O(L.aux);O(L.resv);O(L.list);O(L.prod);O(L.blist);O(L.blist0);O(L.snap);O(L.outw);O(L.outm);O(L.wall);O(L.ballot);O(L.posbits);O(L.claim);O(L.vis);O(L.sc)
#define BLL(B) O(B.unit);O(B.uid);O(B.act);O(B.ucell);O(B.uuid);O(B.pa);O(B.aa);O(B.pend);O(B.pab);O(B.vis);O(B.wall);O(B.sc);O(B.fw)
