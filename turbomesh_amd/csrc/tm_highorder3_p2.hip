// K16 at order 2: the 45 instantiations k_stack_elevate<2, K, MAP> (tm_highorder3_kernel.hpp)
#include "tm_highorder3_kernel.hpp"

namespace tmh {
template hipError_t ho3_launch<2>(int K, const Ho3Launch& a, hipStream_t st);
}
