// The role function of tarok_playout_cards_net_versus (tarok_amd/csrc/tarok_device.h: net_versus_role,
// net_versus_viewer_net, net_versus_roles_ok) run on the CPU, g++, for tests/test_net_versus_host.py.  A stand-alone program:
// it prints, for every (viewer, mover, own_rel, opp_rel) in 4 x 4 x 16 x 16 in that order, one digit — the role, or 9 where
// net_versus_roles_ok refuses the pair of sets —, 64 x 16 digits a line; then a line of the sixteen viewer networks; then
// "ok <cases>".  It checks by itself only what needs no model: the role of an accepted pair is 0, 1 or 2, sets outside
// 0..15 are refused, and the role reads the two seats through their difference alone.
#include "hip/hip_runtime.h"
#include "../../tarok_amd/csrc/tarok_device.h"
#include <stdio.h>

int main() {
    long cases = 0;
    for (u32 viewer = 0; viewer < 4; viewer++)
        for (u32 mover = 0; mover < 4; mover++) {
            for (u32 own = 0; own < 16; own++)
                for (u32 opp = 0; opp < 16; opp++) {
                    const bool ok = net_versus_roles_ok((int)own, (int)opp);
                    const u32 r = net_versus_role(viewer, mover, own, opp);
                    if (ok && r > 2u) { printf("FAILED role %u %u %u %u\n", viewer, mover, own, opp); return 1; }
                    if (r != net_versus_role((viewer + 1u) & 3u, (mover + 1u) & 3u, own, opp)) {
                        printf("FAILED shift %u %u %u %u\n", viewer, mover, own, opp);
                        return 1;
                    }
                    putchar(ok ? (int)('0' + r) : '9');
                    cases++;
                }
            putchar('\n');
        }
    for (u32 opp = 0; opp < 16; opp++) putchar((int)('0' + net_versus_viewer_net(opp)));
    putchar('\n');
    const int outside[4][2] = {{16, 0}, {0, 16}, {-1, 0}, {0, -1}};
    for (int k = 0; k < 4; k++)
        if (net_versus_roles_ok(outside[k][0], outside[k][1])) { printf("FAILED range %d\n", k); return 1; }
    printf("ok %ld\n", cases);
    return 0;
}
