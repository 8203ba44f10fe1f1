// K16 at order 3: the 45 instantiations k_stack_elevate<3, K, MAP> (tm_highorder3_kernel.hpp)
#include "tm_highorder3_kernel.hpp"

namespace tmh {
template hipError_t ho3_launch<3>(int K, const Ho3Launch& a, hipStream_t st);
}
